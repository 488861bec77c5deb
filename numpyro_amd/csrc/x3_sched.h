// Compile-time filler placement for the hand-placed schedule of k_logreg_x3 (potential_logreg.hip,
// x3_item SCHED 1).  Plain C++17, no device code: a host program can include it and print a plan.
//
// One wave issues in order.  A 32x32x16 bf16 MFMA holds the SIMD's vector issue for 8 of its 32
// cycles; what a wave issues behind it in the remaining 24 (its "gap") is hidden, anything beyond
// them delays the next MFMA.  The tile step's vector work -- the Bernoulli epilogue, the bf16 split
// of the residual, the U term -- is cut into single operations (Op), grouped into threads (an
// ordered chain each) and dealt to the gaps of a phase's MFMAs by plan(): per gap at most
// BUDGET issue cycles at the prices below and at most one 8-cycle (transcendental) instruction,
// a thread's operations in order, the cross-thread orders (the running sum of |m| in value
// order; a residual pair complete before its split) kept, every thread done by its deadline.
// Where a phase holds more work than that, plan() raises the budget of all its gaps together
// until everything is placed, so the excess is spread and not left in a lump at a deadline.
#pragma once

namespace x3s {

enum Kind : int {
  // Bernoulli epilogue of one value v (x3_epi_one, one instruction each):
  EXP,   // e = exp2(-|m|)
  ONE,   // ope = e + 1
  PROD,  // prod[v & 1] *= ope
  LIN,   // lin += |m|
  RCP,   // 1 / ope
  HALF,  // - 1/2
  SIGN,  // copysign(., m)
  LAB,   // + label: the residual
  // three-term bf16 split of one residual pair (split3's loop body):
  U1,  // first term of both values (one packed conversion)
  E0,  // remainder of the even value (shift, subtract)
  E1,  // remainder of the odd value (mask, subtract)
  U2,
  F0,
  F1,
  U3,
  // the tile's U term (x3_epi_finish):
  FINA,  // lin / 2 and log2 of the product (f32)
  FINB,  // both times ln 2 and the sum, in double
  NKIND
};

constexpr int cost_of(int k) {
  switch (k) {
    case EXP: case RCP: return 8;
    case U1: case U2: case U3: return 5;
    case E0: case E1: case F0: case F1: return 8;
    case FINA: return 16;
    case FINB: return 20;
    default: return 4;
  }
}
constexpr int trans_of(int k) { return (k == EXP || k == RCP || k == FINA) ? 1 : 0; }

struct Op {
  int kind, arg;  // arg: the value 0..15, or 4 half + pair
};

constexpr int MAXG = 24, MAXO = 40, MAXT = 6, MAXL = 72;
constexpr int BUDGET = 24;

struct Thread {
  Op op[MAXL]{};
  int n = 0, pos = 0;
  int first = 0, last = 0;  // the gaps it may use; everything left is placed at `last`
  int leftc = 0;            // issue cycles of the operations not yet placed
  constexpr void add(int k, int a) {
    op[n++] = Op{k, a};
    leftc += cost_of(k);
  }
  constexpr int left() const { return leftc; }
};

struct Plan {
  int ngaps = 0;
  int n[MAXG]{};
  Op op[MAXG][MAXO]{};
  int cost[MAXG]{}, trans[MAXG]{};
  int budget = 0, tlimit = 0;      // the limits this plan was made at
  int maxcost = 0, maxtrans = 0;  // the fullest gap
  int over = 0;                    // issue cycles placed beyond BUDGET, all gaps
  bool ok = true;                  // every operation placed
};

// the epilogue operations of value v, label add included or not
constexpr void add_value(Thread& t, int v, bool label) {
  t.add(EXP, v);
  t.add(ONE, v);
  t.add(PROD, v);
  t.add(RCP, v);
  t.add(HALF, v);
  t.add(SIGN, v);
  if (label) t.add(LAB, v);
}
constexpr void add_split(Thread& t, int half) {
  for (int p = 0; p < 4; ++p) {
    const int a = 4 * half + p;
    t.add(U1, a);
    t.add(E0, a);
    t.add(E1, a);
    t.add(U2, a);
    t.add(F0, a);
    t.add(F1, a);
    t.add(U3, a);
  }
}

struct State {
  bool lab[16]{};  // residual v complete
  int lin = 0;     // the next value whose |m| the running sum takes
  int lab_hi = 0;  // the labels of the values 8..15 are in registers from this gap on
  constexpr bool ready(const Op& o, int g) const {
    if (o.kind == LIN) return lin == o.arg;
    if (o.kind == LAB && o.arg >= 8) return g >= lab_hi;
    if (o.kind == U1) {
      const int v = 8 * (o.arg >> 2) + 2 * (o.arg & 3);
      return lab[v] && lab[v + 1];
    }
    return true;
  }
  constexpr void done(const Op& o) {
    if (o.kind == LIN) lin = o.arg + 1;
    if (o.kind == LAB) lab[o.arg] = true;
  }
};

// one pass at a given budget and transcendental limit per gap
constexpr Plan plan_at(const Thread (&th0)[MAXT], int nth, int ngaps, State st, int budget, int tlimit) {
  Thread th[MAXT];
  for (int t = 0; t < nth; ++t) th[t] = th0[t];
  Plan pl;
  pl.ngaps = ngaps;
  pl.budget = budget;
  pl.tlimit = tlimit;
  for (int g = 0; g < ngaps; ++g) {
    // a thread's fair share of this gap: what it has left over the gaps it may still use
    int quota[MAXT]{}, given[MAXT]{};
    for (int t = 0; t < nth; ++t)
      if (g >= th[t].first && g <= th[t].last) quota[t] = (th[t].left() + th[t].last - g) / (th[t].last - g + 1);
    while (true) {
      int best = -1;
      long bestu = -1;
      for (int t = 0; t < nth; ++t) {
        const Thread& T = th[t];
        if (T.pos >= T.n || g < T.first) continue;
        const Op o = T.op[T.pos];
        if (!st.ready(o, g)) continue;
        const bool forced = g >= T.last;
        const int c = cost_of(o.kind);
        if (!forced && (pl.cost[g] + c > budget || pl.trans[g] + trans_of(o.kind) > tlimit)) continue;
        // forced first, then threads still short of their share (the most urgent first), then the rest
        long u = (long)T.left() * 1000 / (T.last - g + 1);
        if (given[t] < quota[t]) u += 100000000L;
        if (forced) u += 1000000000L;
        if (u > bestu) {
          bestu = u;
          best = t;
        }
      }
      if (best < 0) break;
      if (pl.n[g] >= MAXO) {
        pl.ok = false;
        break;
      }
      Thread& T = th[best];
      const Op o = T.op[T.pos++];
      pl.op[g][pl.n[g]++] = o;
      pl.cost[g] += cost_of(o.kind);
      pl.trans[g] += trans_of(o.kind);
      given[best] += cost_of(o.kind);
      T.leftc -= cost_of(o.kind);
      st.done(o);
    }
    if (pl.cost[g] > pl.maxcost) pl.maxcost = pl.cost[g];
    if (pl.trans[g] > pl.maxtrans) pl.maxtrans = pl.trans[g];
    if (pl.cost[g] > BUDGET) pl.over += pl.cost[g] - BUDGET;
  }
  for (int t = 0; t < nth; ++t)
    if (th[t].pos < th[t].n) pl.ok = false;
  return pl;
}

// The placement: within BUDGET and one transcendental per gap where the phase's work allows it;
// where it does not, the smallest per-gap budget (then a second transcendental) at which
// everything is placed without a lump at a deadline, so the excess is spread over the gaps.
constexpr Plan plan(const Thread (&th)[MAXT], int nth, int ngaps, State st) {
  for (int budget = BUDGET; budget < 4 * BUDGET; ++budget)
    for (int tlimit = 1; tlimit <= 2; ++tlimit) {
      // a second transcendental in a gap only once two more cycles per gap have not done it
      const int b = tlimit == 1 ? budget : budget - 2;
      if (b < BUDGET) continue;
      const Plan pl = plan_at(th, nth, ngaps, st, b, tlimit);
      if (pl.ok && pl.maxcost <= b && pl.maxtrans <= tlimit) return pl;
    }
  Plan bad;
  bad.ok = false;
  return bad;
}

// Phase 1, the gaps of GEMM1(k+1): the rest of tile k's epilogue (values rot..15; the first rot
// were rotated into the previous step's phase 2 and only take their labels here) and the first
// split half.  Even and odd values are threads of their own (two independent chains in flight).
constexpr Plan plan1(int rot, int ngaps, int split_from, int lab_hi) {
  Thread th[MAXT];
  for (int v = rot; v < 16; ++v) add_value(th[v & 1], v, true);
  for (int v = rot; v < 16; ++v) th[4].add(LIN, v);
  for (int v = 0; v < rot && v < 8; ++v) th[2].add(LAB, v);
  add_split(th[2], 0);
  for (int v = 8; v < rot; ++v) th[3].add(LAB, v);
  for (int t = 0; t < 5; ++t) th[t].last = ngaps - 1;
  // the labels of the rotated values first (their label registers are free after that); the split
  // from gap split_from on (its 12 result registers and its temporaries come late, when most of
  // the accumulator and the labels are dead: the register budget)
  th[2].last = th[3].last = split_from > 0 ? split_from - 1 : 0;
  th[5] = th[2];
  th[2] = Thread{};
  for (int i = 0; i < th[5].n; ++i)
    if (th[5].op[i].kind == LAB) th[2].add(LAB, th[5].op[i].arg);
  Thread sp;
  add_split(sp, 0);
  sp.first = split_from;
  sp.last = ngaps - 1;
  th[5] = sp;
  th[2].last = th[3].last;
  State st;
  st.lin = rot;
  st.lab_hi = lab_hi;
  return plan(th, 6, ngaps, st);
}

// Phase 2, the gaps of GEMM2(k): the second split half (complete before the first MFMA of
// k-step 1, index `split_by`), tile k's U term, and the label-free part of the first rot values
// of tile k+1's epilogue, from gap `acc_from` on (the last GEMM1 MFMA's result is not readable
// before).
constexpr Plan plan2(int rot, int ngaps, int split_by, int acc_from) {
  Thread th[MAXT];
  add_split(th[0], 1);
  th[0].last = split_by - 1;
  th[1].add(FINA, 0);
  th[1].add(FINB, 0);
  th[1].last = ngaps - 1;
  for (int v = 0; v < rot; ++v) add_value(th[2 + (v & 1)], v, false);
  for (int v = 0; v < rot; ++v) th[4].add(LIN, v);
  for (int t = 2; t < 5; ++t) {
    th[t].first = acc_from;
    th[t].last = ngaps - 1;
  }
  State st;
  for (int v = 0; v < 16; ++v) st.lab[v] = true;
  st.lin = 0;
  return plan(th, 5, ngaps, st);
}

}  // namespace x3s

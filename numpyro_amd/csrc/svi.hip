// Stochastic variational inference with a mean-field normal guide: the particle draw, the
// reduction of the potential's gradient over the particles, the optimiser and the loss.
// include/numpyro_amd.h "stochastic variational inference" states the arithmetic.
//
// A step is the potential's own launch over the P particles followed by ONE launch of k_svi_step:
// workgroup b < ceil(D / 4) owns the coordinates of Philox block b, i.e. the rows 4 b .. 4 b + 3 of
// grad, eps and z ([D][ldc], contiguous in the particle).  Wave q < 4 reduces row 4 b + q (lane l adds
// p = l, l + 64, ..., then the xor butterfly: an order fixed by P alone, no atomics) and its lane 0
// applies the optimiser to that coordinate, reading the parameters of step t and writing those of
// step t + 1 (two buffers: no workgroup reads what another has written in this launch).  After a
// barrier the whole workgroup draws the block's normals for step t + 1 -- one Philox block per
// particle gives the four coordinates -- and writes the four rows of eps and z.  The last
// workgroup reduces pe[P] and log scale[D] of step t into the loss.
#include <cmath>

#include "nmx_api_internal.h"
#include "nmx_common.h"

namespace {

constexpr int SVI_THREADS = 1024;  // 16 waves: four reduce a row each, all draw
constexpr int SVI_UNROLL = 8;      // loads in flight per lane of a reduction (the order of the adds is unchanged)
constexpr float SVI_HALF_LOG_2PI_E = 1.4189385332046727f;  // (1 + log 2 pi) / 2

__device__ __forceinline__ float svi_wave_sum(float x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
  return x;
}

__device__ __forceinline__ float svi_softplus(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }

// The four normals of Philox block blk for (particle, iter, event), in the order of the momentum draw.
__device__ __forceinline__ void svi_normals(uint64_t seed, uint32_t particle, uint32_t iter, uint32_t event, int blk,
                                            float n[4]) {
  const nmx_u4 x = nmx_rng(seed, particle, iter, event, (uint32_t)blk, 0u);
  nmx_box_muller(x.x, x.y, n[0], n[1]);
  nmx_box_muller(x.z, x.w, n[2], n[3]);
}

// Rows 4 blk .. 4 blk + 3 of z (and of eps when kept) for the particles p = tid, tid + 1024, ... < P.
__device__ __forceinline__ void svi_draw_block(const nmx_svi_config& cfg, int blk, const float loc[4],
                                               const float scale[4], uint32_t event, uint32_t iter, int64_t offset,
                                               float* __restrict__ z, float* __restrict__ eps) {
  const int P = cfg.num_particles, D = cfg.dim, ldc = cfg.ldc;
  for (int p = threadIdx.x; p < P; p += SVI_THREADS) {
    float n[4];
    svi_normals(cfg.seed, (uint32_t)(offset + p), iter, event, blk, n);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int d = 4 * blk + q;
      if (d < D) {
        NMX_DCHECK(d >= 0 && p >= 0 && p < P && P <= ldc);
        const size_t i = (size_t)d * ldc + p;
        if (eps) eps[i] = n[q];
        z[i] = loc[q] + scale[q] * n[q];
      }
    }
  }
}

__global__ __launch_bounds__(SVI_THREADS) void k_svi_draw(nmx_svi_config cfg, const float* __restrict__ loc,
                                                          const float* __restrict__ scale, uint32_t event,
                                                          uint32_t iter, int64_t offset, float* __restrict__ z,
                                                          float* __restrict__ eps) {
  const int blk = blockIdx.x;
  float l[4], s[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int d = 4 * blk + q;
    NMX_DCHECK(blk >= 0 && 4 * blk < cfg.dim);
    l[q] = d < cfg.dim ? loc[d] : 0.0f;
    s[q] = d < cfg.dim ? scale[d] : 0.0f;
  }
  svi_draw_block(cfg, blk, l, s, event, iter, offset, z, eps);
}

// loss[0] = mean_p pe[p] - sum_d log scale[d] - D / 2 (1 + log 2 pi), by wave 0 of the workgroup
__device__ __forceinline__ void svi_loss(const nmx_svi_config& cfg, const float* __restrict__ par,
                                         const float* __restrict__ pe, float* __restrict__ loss) {
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x, P = cfg.num_particles, D = cfg.dim;
  float u = 0.0f, ls = 0.0f;
  int p = lane;
  for (; p + (SVI_UNROLL - 1) * 64 < P; p += SVI_UNROLL * 64) {
    NMX_DCHECK(p + (SVI_UNROLL - 1) * 64 < cfg.ldc);
    float x[SVI_UNROLL];
#pragma unroll
    for (int k = 0; k < SVI_UNROLL; ++k) x[k] = pe[p + 64 * k];
#pragma unroll
    for (int k = 0; k < SVI_UNROLL; ++k) u += x[k];
  }
  for (; p < P; p += 64) {
    NMX_DCHECK(p < cfg.ldc);
    u += pe[p];
  }
  for (int d = lane; d < D; d += 64) {
    NMX_DCHECK(d >= 0 && d < D);
    ls += logf(par[(size_t)NMX_SVI_SCALE * D + d]);
  }
  u = svi_wave_sum(u);
  ls = svi_wave_sum(ls);
  if (lane == 0) loss[0] = (u / (float)P - ls) - (float)D * SVI_HALF_LOG_2PI_E;
}

__global__ __launch_bounds__(SVI_THREADS) void k_svi_loss(nmx_svi_config cfg, const float* __restrict__ par,
                                                          const float* __restrict__ pe, float* __restrict__ loss) {
  svi_loss(cfg, par, pe, loss);
}

__global__ __launch_bounds__(SVI_THREADS) void k_svi_step(nmx_svi_config cfg, uint32_t step, float c1, float c2,
                                                          const float* __restrict__ cur, float* __restrict__ nxt,
                                                          const float* __restrict__ grad,
                                                          const float* __restrict__ pe, float* __restrict__ z,
                                                          float* __restrict__ eps, float* __restrict__ loss) {
  const int D = cfg.dim, P = cfg.num_particles, ldc = cfg.ldc;
  const int nblk = (D + 3) >> 2;
  const int blk = blockIdx.x;
  if (blk == nblk) {
    svi_loss(cfg, cur, pe, loss);
    return;
  }
  NMX_DCHECK(blk >= 0 && blk < nblk);
  __shared__ float new_loc[4], new_scale[4];
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int d = 4 * blk + q;
  if (q < 4 && d < D) {  // waves 4 .. 15 wait at the barrier
    const float* __restrict__ g_row = grad + (size_t)d * ldc;
    const float* __restrict__ e_row = eps + (size_t)d * ldc;
    float s1 = 0.0f, s2 = 0.0f;
    int p = lane;
    for (; p + (SVI_UNROLL - 1) * 64 < P; p += SVI_UNROLL * 64) {
      NMX_DCHECK(p + (SVI_UNROLL - 1) * 64 < ldc);
      float g[SVI_UNROLL], e[SVI_UNROLL];
#pragma unroll
      for (int k = 0; k < SVI_UNROLL; ++k) {
        g[k] = g_row[p + 64 * k];
        e[k] = e_row[p + 64 * k];
      }
#pragma unroll
      for (int k = 0; k < SVI_UNROLL; ++k) {
        s1 += g[k];
        s2 += g[k] * e[k];
      }
    }
    for (; p < P; p += 64) {
      NMX_DCHECK(p < ldc);
      const float g = g_row[p];
      s1 += g;
      s2 += g * e_row[p];
    }
    s1 = svi_wave_sum(s1);
    s2 = svi_wave_sum(s2);
    if (lane == 0) {
      NMX_DCHECK(d >= 0 && d < D && q < 4);  // the parameter rows are [NMX_SVI_ROWS][D]
#define PAR(buf, row) buf[(size_t)(row) * D + d]
      float loc = PAR(cur, NMX_SVI_LOC), rho = PAR(cur, NMX_SVI_RHO);
      const float scale = PAR(cur, NMX_SVI_SCALE);
      const float g_loc = s1 / (float)P;
      const float g_scale = s2 / (float)P - 1.0f / scale;
      const float g_rho = g_scale * nmx_sigmoid(rho);
      if (cfg.optimizer == NMX_SVI_ADAM) {
        const float b1 = cfg.b1, b2 = cfg.b2;
        const float m_loc = (1.0f - b1) * g_loc + b1 * PAR(cur, NMX_SVI_M_LOC);
        const float v_loc = (1.0f - b2) * (g_loc * g_loc) + b2 * PAR(cur, NMX_SVI_V_LOC);
        const float m_rho = (1.0f - b1) * g_rho + b1 * PAR(cur, NMX_SVI_M_RHO);
        const float v_rho = (1.0f - b2) * (g_rho * g_rho) + b2 * PAR(cur, NMX_SVI_V_RHO);
        loc -= cfg.step_size * (m_loc / c1) / (sqrtf(v_loc / c2) + cfg.eps);
        rho -= cfg.step_size * (m_rho / c1) / (sqrtf(v_rho / c2) + cfg.eps);
        PAR(nxt, NMX_SVI_M_LOC) = m_loc;
        PAR(nxt, NMX_SVI_V_LOC) = v_loc;
        PAR(nxt, NMX_SVI_M_RHO) = m_rho;
        PAR(nxt, NMX_SVI_V_RHO) = v_rho;
      } else {
        loc -= cfg.step_size * g_loc;
        rho -= cfg.step_size * g_rho;
      }
      const float sc = svi_softplus(rho);
      PAR(nxt, NMX_SVI_LOC) = loc;
      PAR(nxt, NMX_SVI_RHO) = rho;
      PAR(nxt, NMX_SVI_SCALE) = sc;
#undef PAR
      new_loc[q] = loc;
      new_scale[q] = sc;
    }
  }
  __syncthreads();  // the rows of eps are read above by their waves and rewritten below by every thread
  float l[4], s[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    l[k] = 4 * blk + k < D ? new_loc[k] : 0.0f;
    s[k] = 4 * blk + k < D ? new_scale[k] : 0.0f;
  }
  svi_draw_block(cfg, blk, l, s, NMX_EV_SVI, step + 1u, 0, z, eps);
}

int svi_check(const nmx_svi_config* cfg, const char* what) {
  if (!cfg) return nmx_fail(NMX_ERR_INVALID, "%s: NULL config", what);
  if (cfg->dim < 1 || cfg->dim > (1 << 26))
    return nmx_fail(NMX_ERR_INVALID, "%s: dim = %d outside [1, 2^26] (the counter's block field is 24 bits)", what,
                    cfg->dim);
  if (cfg->num_particles < 1) return nmx_fail(NMX_ERR_INVALID, "%s: num_particles = %d", what, cfg->num_particles);
  if (cfg->ldc < cfg->num_particles || cfg->ldc % 64 != 0)
    return nmx_fail(NMX_ERR_INVALID, "%s: ldc = %d, need a multiple of 64 >= num_particles = %d", what, cfg->ldc,
                    cfg->num_particles);
  return NMX_OK;
}

}  // namespace

extern "C" int nmx_svi_draw(const nmx_svi_config* cfg, const float* loc, const float* scale, int event, uint32_t iter,
                            int64_t particle_offset, float* z, float* eps_out, void* stream) {
  if (const int st = svi_check(cfg, "svi_draw")) return st;
  if (!loc || !scale || !z) return nmx_fail(NMX_ERR_INVALID, "svi_draw: NULL loc, scale or z");
  if (event != NMX_SVI_EVENT_STEP && event != NMX_SVI_EVENT_GUIDE)
    return nmx_fail(NMX_ERR_INVALID, "svi_draw: event = %d, need NMX_SVI_EVENT_STEP or NMX_SVI_EVENT_GUIDE", event);
  if (particle_offset < 0 || particle_offset + cfg->num_particles > ((int64_t)1 << 32))
    return nmx_fail(NMX_ERR_INVALID, "svi_draw: particles [%lld, +%d) leave the 32-bit counter word",
                    (long long)particle_offset, cfg->num_particles);
  const int nblk = (cfg->dim + 3) / 4;
  hipLaunchKernelGGL(k_svi_draw, dim3(nblk), dim3(SVI_THREADS), 0, (hipStream_t)stream, *cfg, loc, scale,
                     (uint32_t)event, iter, particle_offset, z, eps_out);
  return nmx_check_launch("k_svi_draw");
}

extern "C" int nmx_svi_step(const nmx_svi_config* cfg, int step, const float* par_cur, float* par_next,
                            const float* grad, const float* pe, float* z, float* eps, float* loss, void* stream) {
  if (const int st = svi_check(cfg, "svi_step")) return st;
  if (!par_cur || !par_next || !grad || !pe || !z || !eps || !loss)
    return nmx_fail(NMX_ERR_INVALID, "svi_step: NULL par_cur, par_next, grad, pe, z, eps or loss");
  const size_t par_floats = (size_t)NMX_SVI_ROWS * cfg->dim;
  if (par_cur < par_next + par_floats && par_next < par_cur + par_floats)
    return nmx_fail(NMX_ERR_INVALID, "svi_step: par_cur and par_next overlap");
  if (step < 0 || step == INT32_MAX) return nmx_fail(NMX_ERR_INVALID, "svi_step: step = %d", step);
  if (cfg->optimizer != NMX_SVI_SGD && cfg->optimizer != NMX_SVI_ADAM)
    return nmx_fail(NMX_ERR_INVALID, "svi_step: optimizer = %d, need NMX_SVI_SGD or NMX_SVI_ADAM", cfg->optimizer);
  float c1 = 1.0f, c2 = 1.0f;
  if (cfg->optimizer == NMX_SVI_ADAM) {
    if (!(cfg->b1 >= 0.0f && cfg->b1 < 1.0f && cfg->b2 >= 0.0f && cfg->b2 < 1.0f))
      return nmx_fail(NMX_ERR_INVALID, "svi_step: Adam b1 = %g, b2 = %g outside [0, 1)", cfg->b1, cfg->b2);
    c1 = (float)(1.0 - std::pow((double)cfg->b1, (double)step + 1.0));
    c2 = (float)(1.0 - std::pow((double)cfg->b2, (double)step + 1.0));
  }
  const int nblk = (cfg->dim + 3) / 4;
  hipLaunchKernelGGL(k_svi_step, dim3(nblk + 1), dim3(SVI_THREADS), 0, (hipStream_t)stream, *cfg, (uint32_t)step, c1,
                     c2, par_cur, par_next, grad, pe, z, eps, loss);
  return nmx_check_launch("k_svi_step");
}

extern "C" int nmx_svi_loss(const nmx_svi_config* cfg, const float* par, const float* pe, float* loss, void* stream) {
  if (const int st = svi_check(cfg, "svi_loss")) return st;
  if (!par || !pe || !loss) return nmx_fail(NMX_ERR_INVALID, "svi_loss: NULL par, pe or loss");
  hipLaunchKernelGGL(k_svi_loss, dim3(1), dim3(SVI_THREADS), 0, (hipStream_t)stream, *cfg, par, pe, loss);
  return nmx_check_launch("k_svi_loss");
}

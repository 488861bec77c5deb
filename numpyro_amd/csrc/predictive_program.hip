// Predictive programs: posterior and prior predictive draws of any traced model in the program
// compiler's class (numpyro/infer/util.py:803-885 _predictive: the model re-run with the given
// sites substituted from each posterior sample and the other sites sampled).  One wave (a
// 64-thread workgroup) per posterior sample interprets the forward-only program with its draw
// ops (per-sample body and the draws' word assignment in nmx_program.h, the format in
// include/numpyro_amd.h "predictive programs"); the host reads the output sites as slices of the
// tape.  nmx_predict_program_check validates a program on the host before it may be uploaded,
// so every address the kernel forms comes from checked fields.
#include "nmx_api_internal.h"
#include "nmx_common.h"
#include "nmx_program.h"

namespace {

// 6 waves / SIMD is the kernel's occupancy since the binomial draw (80 VGPRs, nmx_program.h
// nmx_draw_binomial).  The cumsum / logsumexp / concat cases of NmxProgram::forward made the
// allocator take 87 VGPRs (5 waves) although no path needs more than 80; with the occupancy
// stated it allocates 80 again, without a spill or scratch (DESIGN.md "Simplex latents").
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6))) void k_program_predict(NmxPredict pr, const float* __restrict__ samples,
                                                        int num_samples, uint32_t sample_offset,
                                                        float* __restrict__ tape) {
  const int row = blockIdx.x;
  if (row >= num_samples) return;
  pr(samples, tape, row, sample_offset + (uint32_t)row, threadIdx.x);
}

}  // namespace

extern "C" int nmx_predict_program_check(const nmx_program* hp, const int32_t* outputs, int num_outputs) {
  return nmx_program_check_impl(hp, true, outputs, num_outputs);
}

extern "C" size_t nmx_predict_program_workspace_bytes(int num_slots, int num_samples) {
  if (num_slots <= 0 || num_samples <= 0) return 0;
  return (size_t)num_samples * (size_t)num_slots * sizeof(float);
}

extern "C" int nmx_predict_program(const nmx_program* program, const float* samples, int num_samples,
                                   int64_t sample_offset, uint64_t seed, float* tape, void* stream) {
  if (!program || !program->ops || !program->consts || !tape || program->num_ops <= 0 || program->dim < 0 ||
      program->num_slots <= program->dim || (program->num_index > 0 && !program->index))
    return nmx_fail(NMX_ERR_INVALID, "predict_program: bad program or tape");
  if (program->dim > 0 && !samples) return nmx_fail(NMX_ERR_INVALID, "predict_program: NULL samples with dim %d", program->dim);
  // the sample index is one 32-bit counter word
  if (num_samples <= 0 || sample_offset < 0 || sample_offset + num_samples > 0xFFFFFFFFll)
    return nmx_fail(NMX_ERR_INVALID, "predict_program: bad num_samples / sample_offset (%d / %lld)", num_samples,
                    (long long)sample_offset);
  hipLaunchKernelGGL(k_program_predict, dim3(num_samples), dim3(64), 0, (hipStream_t)stream,
                     NmxPredict{NmxProgram{*program, nullptr}, seed}, samples, num_samples, (uint32_t)sample_offset,
                     tape);
  return nmx_check_launch("k_program_predict");
}

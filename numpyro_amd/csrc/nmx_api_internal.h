// Error plumbing shared by the C-ABI entry points (status codes of include/numpyro_amd.h).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/numpyro_amd.h"

int nmx_fail(int code, const char* fmt, ...);
int nmx_check_launch(const char* what);
// Raise `fn`'s dynamic-LDS limit to `bytes` on the device of `stream` (once per kernel and
// device; no-op at <= 64 KiB).  Returns NMX_OK or a status with nmx_last_error set.
int nmx_lds_limit(const void* fn, size_t bytes, hipStream_t stream, const char* what);
// nmx_program_check / nmx_predict_program_check (potential_program.hip): one check for both
// program kinds; `outputs` (num_outputs x { slot, n }) only for a predictive program.
int nmx_program_check_impl(const nmx_program* host_program, bool predictive, const int32_t* outputs, int num_outputs);

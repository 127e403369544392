// The reference's TF batch norm + activation as the ConvNet's row entries end in it — cbl_unary_layer_*, cbl_up_conv_* (through unary_tile.h) and
// cbl_pool_bn_* (pool_bn.hip) — stated ONCE: for z (rows, C), whether a product's result or an input,
//   bn_mode 0: none.  1: batch statistics, the BIASED variance (tf.nn.moments); save_mean / save_invstd = 1 / sqrt(var + eps) are written, and the moving
//              statistics, where given (both or neither), become moving * momentum + batch * (1 - momentum).  2: the moving statistics are the ones used
//              (and written to save_mean / save_invstd); they stay as they are.
//   out      : act(xhat * gamma + beta), xhat = (z - mean) * invstd in ONE association (tfbn_xhat) wherever it is taken; activation 0 none, 1 relu,
//              2 leaky_relu(0.2) (pair_act / pair_dact, the slope read from the OUTPUT: out > 0 exactly where its input was).
//   backward : dz = grad_out * act'(out); grad_beta = sum dz, grad_gamma = sum dz * xhat (fp64, block partials summed in block order:
//              tfbn_sums_finalize_kernel); through bn_mode 1 dz becomes gamma invstd ((dz - sum dz / N) - xhat sum dz xhat / N), through bn_mode 2 gamma invstd dz.
//   pointers : tfbn_check_forward / tfbn_check_backward say which may be NULL.  Whatever else an entry needs (its rows, the y of a product) it checks itself.
// Only what was the same text in those files is here: their statistics schemes, element passes and argument structs differ and stay with them.  Every kernel
// lives in an unnamed namespace: each translation unit holds its own instances, as with pair_tile.h.
#pragma once
#include "pair_tile.h"                                            // pair_f32x4

namespace {

constexpr int TFBN_BLOCK = 256;                                     // threads of the two kernels here: a thread per column

// four columns of a row from p: one 16-byte access (vec), or the nv < 4 valid ones singly, the others zero
__device__ __forceinline__ pair_f32x4 tfbn_ld4(const float* __restrict__ p, bool vec, int nv)
{
    if (vec) return *reinterpret_cast<const pair_f32x4*>(p);
    pair_f32x4 t = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; q++) if (q < nv) t[q] = p[q];
    return t;
}
__device__ __forceinline__ void tfbn_st4(float* __restrict__ p, pair_f32x4 v, bool vec, int nv)
{
    if (vec) { *reinterpret_cast<pair_f32x4*>(p) = v; return; }
#pragma unroll
    for (int q = 0; q < 4; q++) if (q < nv) p[q] = v[q];
}

__device__ __forceinline__ float tfbn_xhat(float z, float mean, float invstd) { return (z - mean) * invstd; }
__device__ __forceinline__ float tfbn_moving_invstd(float var, float eps) { return (float)(1.0 / sqrt((double)var + (double)eps)); }

// what the statistics (N, mean, m2 = the sum of squares about the mean) of column c become: save_mean / save_invstd (also returned: fm, fi), the moving
// statistics the TF way
__device__ __forceinline__ void tfbn_finish_stats(int c, double N, double mean, double m2, float eps, float momentum, float* moving_mean, float* moving_var,
                                                  float* save_mean, float* save_invstd, float& fm, float& fi)
{
    const double var = m2 / N;                                      // biased (tf.nn.moments)
    const float fv = (float)var;
    fm = (float)mean;
    fi = (float)(1.0 / sqrt(var + (double)eps));
    save_mean[c] = fm;
    save_invstd[c] = fi;
    if (moving_mean) moving_mean[c] = moving_mean[c] * momentum + fm * (1.f - momentum);
    if (moving_var) moving_var[c] = moving_var[c] * momentum + fv * (1.f - momentum);
}

// bn_mode 2: the statistics used are the moving ones.  Grid: cbl_div_up(C, TFBN_BLOCK)
__global__ __launch_bounds__(TFBN_BLOCK) void tfbn_moving_stats_kernel(int C, const float* __restrict__ moving_mean, const float* __restrict__ moving_var, float eps,
                                                                        float* __restrict__ save_mean, float* __restrict__ save_invstd)
{
    const int c = blockIdx.x * TFBN_BLOCK + threadIdx.x;
    if (c >= C) return;
    save_mean[c] = moving_mean[c];
    save_invstd[c] = tfbn_moving_invstd(moving_var[c], eps);
}

// backward: the blocks' partials part (nblocks, C, 2) of sum dz and sum dz * xhat, summed in block order -> sums (2, C) (what the element pass reads),
// grad_beta, grad_gamma.  Grid: cbl_div_up(C, TFBN_BLOCK)
__global__ __launch_bounds__(TFBN_BLOCK) void tfbn_sums_finalize_kernel(int C, int nblocks, const double* __restrict__ part, float* __restrict__ sums,
                                                                         float* __restrict__ grad_beta, float* __restrict__ grad_gamma)
{
    const int c = blockIdx.x * TFBN_BLOCK + threadIdx.x;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll 4
    for (int b = 0; b < nblocks; b++) { s1 += part[((size_t)b * C + c) * 2]; s2 += part[((size_t)b * C + c) * 2 + 1]; }
    sums[c] = (float)s1; sums[C + c] = (float)s2;
    if (grad_beta) grad_beta[c] = (float)s1;
    if (grad_gamma) grad_gamma[c] = (float)s2;
}

// ---------------------------------------------------------------- host side
// An entry checks in this order, and the order is part of what it answers: its sizes and tfbn_modes_ok (CBL_ERR_BAD_ARG), its limits (CBL_ERR_UNSUPPORTED),
// no rows (CBL_OK), its own pointers, then tfbn_check_forward / tfbn_check_backward (CBL_ERR_BAD_ARG), then the workspace (CBL_ERR_WORKSPACE)
inline bool tfbn_modes_ok(int bn_mode, int activation) { return bn_mode >= 0 && bn_mode <= 2 && activation >= 0 && activation <= 2; }
inline int tfbn_check_forward(int bn_mode, const float* gamma, const float* beta, float eps, const float* moving_mean, const float* moving_var,
                              const float* save_mean, const float* save_invstd)
{
    if (bn_mode != 0 && (!gamma || !beta || !save_mean || !save_invstd || !(eps > 0.f))) return CBL_ERR_BAD_ARG;
    if (bn_mode == 2 && (!moving_mean || !moving_var)) return CBL_ERR_BAD_ARG;
    if (bn_mode == 1 && ((moving_mean == nullptr) != (moving_var == nullptr))) return CBL_ERR_BAD_ARG;
    return CBL_OK;
}
inline int tfbn_check_backward(int bn_mode, int activation, const float* gamma, const float* save_mean, const float* save_invstd, const float* out,
                               const float* grad_gamma, const float* grad_beta)
{
    if (activation != 0 && !out) return CBL_ERR_BAD_ARG;
    if (bn_mode != 0 && (!gamma || !save_mean || !save_invstd)) return CBL_ERR_BAD_ARG;
    if (bn_mode == 0 && (grad_gamma || grad_beta)) return CBL_ERR_BAD_ARG;
    return CBL_OK;
}

inline void tfbn_launch_moving_stats(hipStream_t st, int C, const float* moving_mean, const float* moving_var, float eps, float* save_mean, float* save_invstd)
{
    hipLaunchKernelGGL(tfbn_moving_stats_kernel, dim3(cbl_div_up(C, TFBN_BLOCK)), dim3(TFBN_BLOCK), 0, st, C, moving_mean, moving_var, eps, save_mean, save_invstd);
}
inline void tfbn_launch_sums_finalize(hipStream_t st, int C, int nblocks, const double* part, float* sums, float* grad_beta, float* grad_gamma)
{
    hipLaunchKernelGGL(tfbn_sums_finalize_kernel, dim3(cbl_div_up(C, TFBN_BLOCK)), dim3(TFBN_BLOCK), 0, st, C, nblocks, part, sums, grad_beta, grad_gamma);
}

// the workspace base, rounded up to 256 bytes (an entry's plan counts them in)
inline char* tfbn_base(void* ws) { return reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~(uintptr_t)255); }
// rows of width c behind these pointers (NULL: not there) may be taken 16 bytes at a time
inline bool tfbn_vec(int c, const void* p0, const void* p1 = nullptr, const void* p2 = nullptr, const void* p3 = nullptr, const void* p4 = nullptr)
{
    return c % 4 == 0 && cbl_host_aligned16(p0) && cbl_host_aligned16(p1) && cbl_host_aligned16(p2) && cbl_host_aligned16(p3) && cbl_host_aligned16(p4);
}

}  // namespace

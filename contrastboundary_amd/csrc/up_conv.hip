// a15  One decoder step of the ConvNet's segmentation head (tensorflow/models/heads/seg_head.py:63-67): nearest upsample + concat + conv1d_1x1 without the upsampled
//      and the concatenated tensor, forward and backward (cbl_up_conv_*), on the unary layer's kernels (unary_tile.h; described in unary_layer.hip).
// weights (c_up + c_skip, c_out) = [W_up; W_skip], two contiguous row blocks of the one TF variable.  The product is linear, so the gather commutes with it:
//   y[i] = (coarse @ W_up)[idx[i]] + skip[i] @ W_skip (+ biases),   idx[i] = up_inds[i * k]; an id outside [0, n1) is the zero row
// forward : P = coarse @ W_up (n1, c_out) into the workspace (ul_forward_kernel<false>, its epilogue a plain store; where the coarse layer's tiles leave
//           compute units idle, ul_split_product_kernel over splits of the contraction: ul_split_of), then ul_forward_kernel<true> over skip and
//           W_skip, whose epilogue adds P's row; statistics, finalize and the normalise pass as in the unary layer, over the full y.
// backward: column sums and dy on (n2, c_out) as in the unary layer; dyc (n1, c_out) = the sum of dy's rows per coarse row, over the transposed table of the
//           first column in ascending pair order (cbl_grouping_backward_csr_rows: a row nobody references gets zeros); then grad_coarse = dyc @ W_up^T and
//           grad_W_up = coarse^T @ dyc at n1 rows, grad_skip = dy @ W_skip^T and grad_W_skip = skip^T @ dy (+ grad_biases) at n2 rows.
#include "unary_tile.h"

namespace {

// In how many ways the contraction of the plain product (M, K) x (K, N) is split (1: not at all), and the contraction steps of a split.  A rule on the shape
// alone: as many splits as the 64 x 64 tiles fit into the compute units of the device (none once the tiles fill half of them), at most UL_MAX_SPLITS, and no
// split shorter than UL_SPLIT_MIN_PANELS panels
inline int ul_split_of(long long M, int N, int K, int* kspan)
{
    const long long tiles = ((M + UL_T - 1) / UL_T) * ((N + UL_T - 1) / UL_T);
    const int panels = (K + UL_KP - 1) / UL_KP;
    long long s = UL_SPLIT_CUS / tiles;
    if (s > UL_MAX_SPLITS) s = UL_MAX_SPLITS;
    if (s > panels / UL_SPLIT_MIN_PANELS) s = panels / UL_SPLIT_MIN_PANELS;
    *kspan = K;
    if (s < 2) return 1;
    const int per = (int)((panels + s - 1) / s);
    *kspan = per * UL_KP;
    return (panels + per - 1) / per;
}
// measurement knob (tools/bench_up_conv.py --split-ab): CBL_UP_CONV_SPLIT=0 runs the unsplit products whatever the rule says
inline bool ul_split_enabled() { const char* e = getenv("CBL_UP_CONV_SPLIT"); return !(e && e[0] == '0'); }
template <bool B_KC>
inline void ul_launch_split(hipStream_t st, long long M, int N, int K, int splits, int kspan, const float* A, const float* B, float* part, float* out)
{
    UlSplit s;
    s.M = M; s.row_tiles = (M + UL_T - 1) / UL_T; s.N = N; s.K = K; s.kspan = kspan; s.veca = tfbn_vec(K, A); s.vecb = tfbn_vec(B_KC ? K : N, B);
    s.A = A; s.B = B; s.part = part;
    hipLaunchKernelGGL(ul_split_product_kernel<B_KC>, dim3((unsigned)s.row_tiles, cbl_div_up(N, UL_T), splits), dim3(UL_BLOCK), 0, st, s);
    hipLaunchKernelGGL(ul_split_combine_kernel, dim3(cbl_grid_for(M * N, UL_BLOCK)), dim3(UL_BLOCK), 0, st, (size_t)M * N, splits, part, out);
}

struct UpPlan {
    UlPlan skip, up;                                                // the unary plans of (n2, c_skip, c_out) and (n1, c_up, c_out)
    int split_p, kspan_p, split_gc, kspan_gc;                       // ul_split_of coarse @ W_up and of grad_coarse = dyc @ W_up^T
    size_t off_p, off_wpart_up, off_split, bytes;                   // P (forward) and dyc (backward) share (n1, c_out) floats; grad_W_up's own partials; the splits'
};
inline UpPlan up_plan(long long n2, long long n1, int c_up, int c_skip, int c_out)
{
    UpPlan p;
    p.skip = ul_plan(n2, c_skip, c_out);
    p.up = ul_plan(n1, c_up, c_out);
    p.split_p = ul_split_of(n1, c_out, c_up, &p.kspan_p);
    p.split_gc = ul_split_of(n1, c_up, c_out, &p.kspan_gc);
    const size_t split_p = p.split_p > 1 ? (size_t)p.split_p * n1 * c_out : 0, split_gc = p.split_gc > 1 ? (size_t)p.split_gc * n1 * c_up : 0;
    size_t o = p.skip.bytes - 256;
    p.off_p = o;          o += pair_up256((size_t)n1 * c_out * sizeof(float));
    p.off_wpart_up = o;   o += p.up.nchunks > 1 ? pair_up256((size_t)p.up.nchunks * ((size_t)c_up * c_out + c_out) * sizeof(float)) : 0;
    p.off_split = o;      o += pair_up256((split_p > split_gc ? split_p : split_gc) * sizeof(float));
    p.bytes = o + 256;
    return p;
}
// 0, or the code the entries return before any launch
inline int up_check(long long n2, long long n1, int c_up, int c_skip, int c_out, int k)
{
    if (n2 < 0 || n1 < 1 || c_up < 1 || c_skip < 1 || c_out < 1 || k < 1) return CBL_ERR_BAD_ARG;
    if (n2 * (long long)k > 0x7fffffffLL || n1 > 0x7fffffffLL) return CBL_ERR_BAD_ARG;
    if ((long long)c_up + c_skip > UL_MAX_C || c_out > UL_MAX_C) return CBL_ERR_UNSUPPORTED;
    return CBL_OK;
}

}  // namespace

CBL_EXPORT size_t cbl_up_conv_workspace_bytes(long long n2, long long n1, int c_up, int c_skip, int c_out)
{
    if (up_check(n2, n1, c_up, c_skip, c_out, 1) != CBL_OK) return 0;
    return up_plan(n2, n1, c_up, c_skip, c_out).bytes;
}

CBL_EXPORT int cbl_up_conv_forward(long long n2, long long n1, int c_up, int c_skip, int c_out, const float* coarse, const int* up_inds, int k, const float* skip,
                                   const float* weights, const float* biases, int bn_mode, const float* gamma, const float* beta, float eps, float momentum,
                                   float* moving_mean, float* moving_var, int activation, float* save_mean, float* save_invstd, float* y, float* out,
                                   void* workspace, size_t workspace_bytes, void* stream)
{
    if (!tfbn_modes_ok(bn_mode, activation)) return CBL_ERR_BAD_ARG;
    if (const int rc = up_check(n2, n1, c_up, c_skip, c_out, k)) return rc;
    if (n2 == 0) return CBL_OK;
    if (!coarse || !up_inds || !skip || !weights || !out || (bn_mode != 0 && !y)) return CBL_ERR_BAD_ARG;
    if (const int rc = tfbn_check_forward(bn_mode, gamma, beta, eps, moving_mean, moving_var, save_mean, save_invstd)) return rc;
    const UpPlan p = up_plan(n2, n1, c_up, c_skip, c_out);
    if (!workspace || workspace_bytes < p.bytes) return CBL_ERR_WORKSPACE;
    hipStream_t st = cbl_stream(stream);
    char* base = tfbn_base(workspace);
    float* P = reinterpret_cast<float*>(base + p.off_p);
    const float* w_skip = weights + (size_t)c_up * c_out;           // (c_up * c_out may be no multiple of 4: then the scalar-load path)
    if (bn_mode == 2) tfbn_launch_moving_stats(st, c_out, moving_mean, moving_var, eps, save_mean, save_invstd);
    const unsigned col_tiles = cbl_div_up(c_out, UL_T);
    UlForward f = {};
    f.cout = c_out;
    if (p.split_p > 1 && ul_split_enabled())
        ul_launch_split<false>(st, n1, c_out, c_up, p.split_p, p.kspan_p, coarse, weights, reinterpret_cast<float*>(base + p.off_split), P);
    else {
        f.rows = n1; f.row_tiles = p.up.row_tiles; f.cin = c_up;
        f.veca = tfbn_vec(c_up, coarse); f.vecb = tfbn_vec(c_out, weights);
        f.fuse = 1; f.bn = 0; f.act = 0;
        f.x = coarse; f.w = weights; f.out = P;
        hipLaunchKernelGGL(ul_forward_kernel<false>, dim3((unsigned)(f.row_tiles > UL_ROW_BLOCKS ? UL_ROW_BLOCKS : f.row_tiles), col_tiles), dim3(UL_BLOCK), 0, st, f);
    }
    f.rows = n2; f.row_tiles = p.skip.row_tiles; f.cin = c_skip;
    f.veca = tfbn_vec(c_skip, skip); f.vecb = tfbn_vec(c_out, w_skip);
    f.fuse = bn_mode != 1; f.bn = bn_mode != 0; f.act = activation;
    f.x = skip; f.w = w_skip; f.bias = biases; f.mean = save_mean; f.invstd = save_invstd; f.gamma = gamma; f.beta = beta;
    f.y = y; f.out = out; f.part = bn_mode == 1 ? reinterpret_cast<float*>(base + p.skip.off_part) : nullptr;
    f.up_p = P; f.up_idx = up_inds; f.up_n1 = n1; f.up_k = k;
    hipLaunchKernelGGL(ul_forward_kernel<true>, dim3((unsigned)(f.row_tiles > UL_ROW_BLOCKS ? UL_ROW_BLOCKS : f.row_tiles), col_tiles), dim3(UL_BLOCK), 0, st, f);
    if (bn_mode == 1)
        ul_launch_bn_tail(st, n2, c_out, p.skip.row_tiles, f.part, eps, momentum, moving_mean, moving_var, save_mean, save_invstd, gamma, beta, activation, y, nullptr, out);
    return cbl_status();
}

CBL_EXPORT int cbl_up_conv_backward(long long n2, long long n1, int c_up, int c_skip, int c_out, const float* coarse, const int* up_inds, int k, const float* skip,
                                    const float* weights, int bn_mode, const float* gamma, const float* save_mean, const float* save_invstd, int activation,
                                    const float* y, const float* out, const float* grad_out, const int* order, const int* inv_start, const int* inv_src,
                                    float* grad_coarse, float* grad_skip, float* grad_weights, float* grad_biases, float* grad_gamma, float* grad_beta,
                                    void* workspace, size_t workspace_bytes, void* stream)
{
    (void)up_inds;                                                  // the backward pass walks the transposed table, never the table itself
    if (!tfbn_modes_ok(bn_mode, activation)) return CBL_ERR_BAD_ARG;
    if (const int rc = up_check(n2, n1, c_up, c_skip, c_out, k)) return rc;
    if (n2 == 0) return CBL_OK;
    if (!coarse || !skip || !weights || !grad_out || (bn_mode != 0 && !y)) return CBL_ERR_BAD_ARG;
    if (const int rc = tfbn_check_backward(bn_mode, activation, gamma, save_mean, save_invstd, out, grad_gamma, grad_beta)) return rc;
    const bool coarse_side = grad_coarse || grad_weights;
    if (coarse_side && (!inv_start || !inv_src)) return CBL_ERR_BAD_ARG;
    const UpPlan p = up_plan(n2, n1, c_up, c_skip, c_out);
    if (!workspace || workspace_bytes < p.bytes) return CBL_ERR_WORKSPACE;
    hipStream_t st = cbl_stream(stream);
    char* base = tfbn_base(workspace);
    float* sums = reinterpret_cast<float*>(base + p.skip.off_sums);
    const bool products = coarse_side || grad_skip || grad_biases;
    if (bn_mode == 1 ? (products || grad_gamma || grad_beta) : (grad_gamma || grad_beta))
        ul_launch_colsums(st, n2, c_out, activation, grad_out, out, y, save_mean, save_invstd, p.skip.sum_blocks,
                          reinterpret_cast<double*>(base + p.skip.off_sumpart), sums, grad_beta, grad_gamma);
    if (!products) return cbl_status();
    const bool identity = bn_mode == 0 && activation == 0;
    const float* dy = identity ? grad_out : reinterpret_cast<float*>(base + p.skip.off_dy);
    if (!identity)
        ul_launch_dy(st, n2, c_out, bn_mode, activation, grad_out, out, y, save_mean, save_invstd, gamma, sums, const_cast<float*>(dy), nullptr);
    const float* w_skip = weights + (size_t)c_up * c_out;
    if (coarse_side) {
        float* dyc = reinterpret_cast<float*>(base + p.off_p);
        if (const int rc = cbl_grouping_backward_csr_rows((int)n1, c_out, c_out, 0, dy, order, inv_start, inv_src, dyc, stream)) return rc;
        if (grad_coarse && p.split_gc > 1 && ul_split_enabled())
            ul_launch_split<true>(st, n1, c_up, c_out, p.split_gc, p.kspan_gc, dyc, weights, reinterpret_cast<float*>(base + p.off_split), grad_coarse);
        else if (grad_coarse) ul_launch_dgrad(st, n1, c_up, c_out, dyc, weights, grad_coarse);
        if (grad_weights) ul_launch_wgrad(st, p.up, n1, c_up, c_out, coarse, dyc, grad_weights, nullptr, reinterpret_cast<float*>(base + p.off_wpart_up));
    }
    if (grad_skip) ul_launch_dgrad(st, n2, c_skip, c_out, dy, w_skip, grad_skip);
    if (grad_weights || grad_biases)
        ul_launch_wgrad(st, p.skip, n2, c_skip, c_out, skip, dy, grad_weights ? grad_weights + (size_t)c_up * c_out : nullptr, grad_biases,
                        reinterpret_cast<float*>(base + p.skip.off_wpart));
    return cbl_status();
}

// a15  The ConvNet's unary layer conv1d_1x1 (tensorflow/models/basic_operators.py:195-241): for x (rows, c_in), weights (c_in, c_out) in TF's (in, out) order
//     y = x @ weights (+ biases),   z = bn(y) (+ shortcut),   out = act(z)
// forward and backward, any 1 <= c_in, c_out <= 4096 and any number of rows.
//   products : the forward product, grad_x = dy @ weights^T and grad_weights = x^T @ dy are ONE tile product (ul_tile_product) on v_mfma_f32_16x16x4_f32: a
//              workgroup of four waves owns a 64 x 64 output tile, wave w its rows 16 w .. 16 w + 15 with four accumulators (the four 16-column tiles: four
//              independent MFMA chains); both operands go through LDS in panels of 64 contraction steps, the next panel's 16-byte loads in flight while this
//              one's MFMAs run (skinny_linear.hip's triple_wide kernels are the pattern).  A panel is 64 x 64 floats of a row-major matrix and is staged
//              as it lies in memory; what differs between the products is only which of the panel's two indices is the contraction index: a k-contiguous
//              operand (x and dy as the left operand, weights in grad_x) has LDS rows of 64 + 4 floats, an operand whose rows ARE the contraction steps
//              (weights in the forward product, x and dy in grad_weights) rows of 64 + 16 floats.  Widths and rows are run-time values: a panel element past
//              an edge is staged as zero, a result past an edge is not stored; rows whose address is not 16-byte aligned (c % 4 != 0 or an unaligned base)
//              are read with scalar loads.
//   bn_mode 1: the forward product's epilogue leaves per (64-row tile, column) the tile's mean and its CENTRED sum of squares; ul_stats_finalize_kernel
//              combines them in fp64 in tile order (no E[y^2] - E[y]^2 anywhere), writes save_mean / save_invstd and updates the moving statistics the TF
//              way; a second pass normalises, adds the shortcut and applies the activation.  bn_mode 0 / 2: the epilogue itself finishes `out`.
//   backward : one streaming pass for the two column sums sum dz and sum dz * xhat (fp64, block partials summed in block order: grad_beta, grad_gamma), one
//              pass that writes dy (rows, c_out) into the workspace ONCE (and grad_shortcut = dz), then the two products read dy as a plain operand.
//              grad_weights over chunks of rows (at most ceil(rows / 512) chunks, each a multiple of 64 rows): one chunk stores straight to the output,
//              several store partials that ul_wgrad_combine_kernel sums in chunk order (fp64); the workgroups of the first row tile of grad_weights also
//              sum dy's columns (grad_biases; asked for alone, only that row of tiles is launched).
// No float atomics; every output is stored once in a fixed summation order (the grids depend on the shapes alone); no allocation or synchronisation.
// The kernels and their launch helpers are in unary_tile.h, which up_conv.hip (the segmentation head's decoder step) shares.
#include "unary_tile.h"

CBL_EXPORT size_t cbl_unary_layer_workspace_bytes(long long rows, int c_in, int c_out)
{
    if (rows < 0 || c_in < 1 || c_out < 1 || !ul_dims_ok(c_in, c_out)) return 0;
    return ul_plan(rows, c_in, c_out).bytes;
}

CBL_EXPORT int cbl_unary_layer_forward(long long rows, int c_in, int c_out, const float* x, const float* weights, const float* biases, const float* shortcut,
                                       int bn_mode, const float* gamma, const float* beta, float eps, float momentum, float* moving_mean, float* moving_var,
                                       int activation, float* save_mean, float* save_invstd, float* y, float* out, void* workspace, size_t workspace_bytes,
                                       void* stream)
{
    if (rows < 0 || c_in < 1 || c_out < 1 || !tfbn_modes_ok(bn_mode, activation)) return CBL_ERR_BAD_ARG;
    if (!ul_dims_ok(c_in, c_out)) return CBL_ERR_UNSUPPORTED;
    if (rows == 0) return CBL_OK;
    if (!x || !weights || !out || (bn_mode != 0 && !y)) return CBL_ERR_BAD_ARG;
    if (const int rc = tfbn_check_forward(bn_mode, gamma, beta, eps, moving_mean, moving_var, save_mean, save_invstd)) return rc;
    const UlPlan p = ul_plan(rows, c_in, c_out);
    if (bn_mode == 1 && (!workspace || workspace_bytes < p.bytes)) return CBL_ERR_WORKSPACE;
    hipStream_t st = cbl_stream(stream);
    char* base = tfbn_base(workspace);
    if (bn_mode == 2) tfbn_launch_moving_stats(st, c_out, moving_mean, moving_var, eps, save_mean, save_invstd);
    UlForward f;
    f.rows = rows; f.row_tiles = p.row_tiles; f.cin = c_in; f.cout = c_out;
    f.veca = tfbn_vec(c_in, x); f.vecb = tfbn_vec(c_out, weights);
    f.fuse = bn_mode != 1; f.bn = bn_mode != 0; f.act = activation;
    f.x = x; f.w = weights; f.bias = biases; f.mean = save_mean; f.invstd = save_invstd; f.gamma = gamma; f.beta = beta; f.shortcut = shortcut;
    f.y = y; f.out = out; f.part = bn_mode == 1 ? reinterpret_cast<float*>(base + p.off_part) : nullptr;
    f.up_p = nullptr; f.up_idx = nullptr; f.up_n1 = 0; f.up_k = 0;
    const dim3 grid((unsigned)(p.row_tiles > UL_ROW_BLOCKS ? UL_ROW_BLOCKS : p.row_tiles), cbl_div_up(c_out, UL_T));
    hipLaunchKernelGGL(ul_forward_kernel<false>, grid, dim3(UL_BLOCK), 0, st, f);
    if (bn_mode == 1)
        ul_launch_bn_tail(st, rows, c_out, p.row_tiles, f.part, eps, momentum, moving_mean, moving_var, save_mean, save_invstd, gamma, beta, activation, y, shortcut, out);
    return cbl_status();
}

CBL_EXPORT int cbl_unary_layer_backward(long long rows, int c_in, int c_out, const float* x, const float* weights, int bn_mode, const float* gamma,
                                        const float* save_mean, const float* save_invstd, int activation, const float* y, const float* out,
                                        const float* grad_out, float* grad_x, float* grad_weights, float* grad_biases, float* grad_gamma, float* grad_beta,
                                        float* grad_shortcut, void* workspace, size_t workspace_bytes, void* stream)
{
    if (rows < 0 || c_in < 1 || c_out < 1 || !tfbn_modes_ok(bn_mode, activation)) return CBL_ERR_BAD_ARG;
    if (!ul_dims_ok(c_in, c_out)) return CBL_ERR_UNSUPPORTED;
    if (rows == 0) return CBL_OK;
    if (!x || !weights || !grad_out || (bn_mode != 0 && !y)) return CBL_ERR_BAD_ARG;
    if (const int rc = tfbn_check_backward(bn_mode, activation, gamma, save_mean, save_invstd, out, grad_gamma, grad_beta)) return rc;
    const UlPlan p = ul_plan(rows, c_in, c_out);
    if (!workspace || workspace_bytes < p.bytes) return CBL_ERR_WORKSPACE;
    hipStream_t st = cbl_stream(stream);
    char* base = tfbn_base(workspace);
    float* sums = reinterpret_cast<float*>(base + p.off_sums);
    const bool products = grad_x || grad_weights || grad_biases;
    if (bn_mode == 1 ? (products || grad_gamma || grad_beta) : (grad_gamma || grad_beta)) {
        ul_launch_colsums(st, rows, c_out, activation, grad_out, out, y, save_mean, save_invstd, p.sum_blocks, reinterpret_cast<double*>(base + p.off_sumpart), sums,
                          grad_beta, grad_gamma);
    }
    // dy: grad_out itself where neither a batch norm nor an activation stands between them
    const bool identity = bn_mode == 0 && activation == 0;
    const float* dy = identity ? grad_out : reinterpret_cast<float*>(base + p.off_dy);
    if ((products && !identity) || grad_shortcut)
        ul_launch_dy(st, rows, c_out, bn_mode, activation, grad_out, out, y, save_mean, save_invstd, gamma, sums,
                     (products && !identity) ? const_cast<float*>(dy) : nullptr, grad_shortcut);
    if (grad_x) ul_launch_dgrad(st, rows, c_in, c_out, dy, weights, grad_x);
    if (grad_weights || grad_biases)
        ul_launch_wgrad(st, p, rows, c_in, c_out, x, dy, grad_weights, grad_biases, reinterpret_cast<float*>(base + p.off_wpart));
    return cbl_status();
}

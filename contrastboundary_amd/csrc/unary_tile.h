// The tiled f32 MFMA product, the batch-norm passes and the launch helpers of the ConvNet's unary layer, shared by the two files that run on them:
// unary_layer.hip (cbl_unary_layer_*: conv1d_1x1, where the kernels are described) and up_conv.hip (cbl_up_conv_*: the segmentation head's decoder step, which
// adds the template argument UP of ul_forward_kernel and the split-contraction product).  Every kernel here lives in an unnamed namespace: each of the two
// translation units holds its own instances, as with pair_tile.h.
#pragma once
#include <cstdlib>

#include "tf_bn.h"                                                // the batch norm's conventions, its shared kernels and checks; pair_tile.h: pair_act / pair_dact, pair_f32x4, pair_up256

namespace {

constexpr int UL_BLOCK = 256, UL_T = 64, UL_KP = 64;                // threads, output tile edge, contraction steps of a panel
constexpr int UL_LDK = UL_KP + 4, UL_LDN = UL_T + 16, UL_LDY = UL_T + 1;   // LDS row strides: k-contiguous operand, contraction-major operand, the epilogue's y tile
constexpr int UL_PANEL = UL_T * UL_LDN;                             // floats of one operand's panel (the larger of the two layouts)
constexpr int UL_MAX_C = 4096;
constexpr int UL_ROW_BLOCKS = 2048;                                 // grid cap of the row-tile kernels (forward, grad_x): a workgroup walks tiles blockIdx.x, + gridDim.x, ...
constexpr int UL_WALK_BLOCKS = 1024, UL_SUM_BLOCKS = 512;           // grid caps of the elementwise passes and of the column sums
constexpr int UL_WALK_ITEMS = 2048;                                 // 4-column groups of one trip of an elementwise pass
constexpr int UL_CHUNK_ROWS = 512, UL_MAX_CHUNKS = 256;             // grad_weights: at most ceil(rows / 512) and at most 256 chunks, each a multiple of 64 rows
constexpr size_t UL_PARTIAL_FLOATS = (size_t)1 << 23;               // ... and its partials stay within 32 MB

// 64 x 64 floats of the row-major matrix P (element (r, c) at P[r * ld + c] for r < R, c < C, zero outside) from (r0, c0): 4 x 4 floats per thread
__device__ __forceinline__ void ul_panel_load(const float* __restrict__ P, long long ld, long long r0, long long R, long long c0, long long C, bool vec,
                                              pair_f32x4 (&v)[4])
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int e = threadIdx.x + UL_BLOCK * j, rr = e >> 4, c4 = e & 15;
        const long long r = r0 + rr, c = c0 + 4 * c4;
        pair_f32x4 t = {0.f, 0.f, 0.f, 0.f};
        if (r < R) {
            const float* __restrict__ src = P + r * ld + c;
            if (vec && c + 3 < C) t = *reinterpret_cast<const pair_f32x4*>(src);
            else {
#pragma unroll
                for (int q = 0; q < 4; q++) if (c + q < C) t[q] = src[q];
            }
        }
        v[j] = t;
    }
}
__device__ __forceinline__ void ul_panel_store(float* S, int lds, const pair_f32x4 (&v)[4])
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int e = threadIdx.x + UL_BLOCK * j, rr = e >> 4, c4 = e & 15;
        *reinterpret_cast<pair_f32x4*>(&S[rr * lds + 4 * c4]) = v[j];
    }
}

// acc[t] (the 16 x 16 tile of rows m0 + 16 wave .., columns n0 + 16 t ..) += sum_{kbeg <= k < kend} A(m, k) B(k, n).  A_KC: A(m, k) = A[m * lda + k], else
// A[k * lda + m]; B_KC: B(k, n) = B[n * ldb + k], else B[k * ldb + n].  hook(q) runs once per panel with the panel in LDS (As, Bs), before its MFMAs.
// D[4 (lane / 16) + v][lane % 16] in acc[t][v].  The caller synchronises before it reuses As / Bs.
template <bool A_KC, bool B_KC, class HOOK>
__device__ __forceinline__ void ul_tile_product(const float* __restrict__ A, long long lda, bool veca, const float* __restrict__ B, long long ldb, bool vecb,
                                                long long m0, long long M, long long n0, long long N, long long kbeg, long long kend, float* As, float* Bs,
                                                pair_f32x4 (&acc)[4], HOOK hook)
{
    constexpr int LDA = A_KC ? UL_LDK : UL_LDN, LDB = B_KC ? UL_LDK : UL_LDN;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, kq = lane >> 4;
    const int npanel = (int)((kend - kbeg + UL_KP - 1) / UL_KP);
    pair_f32x4 ra[4], rb[4];
    auto load = [&](int q) {
        const long long k0 = kbeg + (long long)q * UL_KP;
        if (A_KC) ul_panel_load(A, lda, m0, M, k0, kend, veca, ra); else ul_panel_load(A, lda, k0, kend, m0, M, veca, ra);
        if (B_KC) ul_panel_load(B, ldb, n0, N, k0, kend, vecb, rb); else ul_panel_load(B, ldb, k0, kend, n0, N, vecb, rb);
    };
    load(0);
    for (int q = 0; q < npanel; q++) {
        __syncthreads();                                            // the previous panel (or the previous tile's epilogue) is consumed
        ul_panel_store(As, LDA, ra);
        ul_panel_store(Bs, LDB, rb);
        __syncthreads();
        if (q + 1 < npanel) load(q + 1);
        hook(q);
#pragma unroll
        for (int s2 = 0; s2 < UL_KP / 4; s2++) {
            const int k = 4 * s2 + kq;
            const float av = A_KC ? As[(16 * wave + n) * LDA + k] : As[k * LDA + 16 * wave + n];
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const float bv = B_KC ? Bs[(16 * t + n) * LDB + k] : Bs[k * LDB + 16 * t + n];
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[t], 0, 0, 0);
            }
        }
    }
}

// z of one element: the batch norm in ONE association (forward epilogue, normalise pass and xhat of the backward passes agree), then the shortcut
__device__ __forceinline__ float ul_z(float y, bool bn, float mean, float invstd, float gamma, float beta, float sc)
{
    const float z = bn ? tfbn_xhat(y, mean, invstd) * gamma + beta : y;
    return z + sc;
}

struct UlForward {
    long long rows, row_tiles;
    int cin, cout, veca, vecb, fuse, bn, act;
    const float *x, *w, *bias, *mean, *invstd, *gamma, *beta, *shortcut;
    float *y, *out, *part;                                          // part: (row_tiles, cout, 2) = the tile's mean and centred sum of squares per column (bn_mode 1)
    const float* up_p;                                              // UP (cbl_up_conv_forward): element (row, col) adds up_p[up_idx[row * up_k]][col], a row of the
    const int* up_idx;                                              // (up_n1, cout) product of the coarser layer; an id outside [0, up_n1) is the zero row
    long long up_n1;
    int up_k;
};

template <bool UP>
__global__ __launch_bounds__(UL_BLOCK) void ul_forward_kernel(UlForward a)
{
    __shared__ __attribute__((aligned(16))) float As[UL_PANEL];
    __shared__ __attribute__((aligned(16))) float Bs[UL_PANEL];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, kq = lane >> 4;
    const long long n0 = (long long)blockIdx.y * UL_T;
    for (long long rt = blockIdx.x; rt < a.row_tiles; rt += gridDim.x) {
        const long long m0 = rt * UL_T;
        pair_f32x4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; t++) acc[t] = pair_f32x4{0.f, 0.f, 0.f, 0.f};
        ul_tile_product<true, false>(a.x, a.cin, a.veca != 0, a.w, a.cout, a.vecb != 0, m0, a.rows, n0, a.cout, 0, a.cin, As, Bs, acc, [](int) {});
        if (a.part) __syncthreads();                                // every wave is done with the panels: As becomes the y tile
        const float* prow[4] = {nullptr, nullptr, nullptr, nullptr};   // UP: this lane's four rows of up_p (the 16 lanes of a column tile read 64 contiguous bytes)
        if (UP) {
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const long long row = m0 + 16 * wave + 4 * kq + v;
                if (row < a.rows) {
                    const long long id = a.up_idx[row * a.up_k];
                    if (id >= 0 && id < a.up_n1) prow[v] = a.up_p + (size_t)id * a.cout;
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const long long col = n0 + 16 * t + n;
            const bool okc = col < a.cout;
            const float bv = (okc && a.bias) ? a.bias[col] : 0.f;
            float mean = 0.f, invstd = 1.f, gamma = 1.f, beta = 0.f;
            if (a.fuse && a.bn && okc) { mean = a.mean[col]; invstd = a.invstd[col]; gamma = a.gamma[col]; beta = a.beta[col]; }
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const int lr = 16 * wave + 4 * kq + v;
                const long long row = m0 + lr;
                const float val = UP ? (acc[t][v] + ((prow[v] && okc) ? prow[v][col] : 0.f)) + bv : acc[t][v] + bv;
                if (a.part) As[lr * UL_LDY + 16 * t + n] = val;
                if (row < a.rows && okc) {
                    const size_t o = (size_t)row * a.cout + col;
                    if (a.y) a.y[o] = val;
                    if (a.fuse) a.out[o] = pair_act(a.act, ul_z(val, a.bn != 0, mean, invstd, gamma, beta, a.shortcut ? a.shortcut[o] : 0.f));
                }
            }
        }
        if (a.part) {
            // per column of the tile: the mean of its nr valid rows, then the sum of squares about that mean (four row quarters, summed in quarter order)
            float* red = Bs;
            const long long left = a.rows - m0;
            const int nr = left < UL_T ? (int)left : UL_T, c = tid & 63, g = tid >> 6;
            __syncthreads();
            float s = 0.f;
#pragma unroll 4
            for (int i = 0; i < 16; i++) { const int r = 16 * g + i; if (r < nr) s += As[r * UL_LDY + c]; }
            red[g * 64 + c] = s;
            __syncthreads();
            const float mean = (((red[c] + red[64 + c]) + red[128 + c]) + red[192 + c]) / (float)nr;
            float m2 = 0.f;
#pragma unroll 4
            for (int i = 0; i < 16; i++) { const int r = 16 * g + i; if (r < nr) { const float d = As[r * UL_LDY + c] - mean; m2 += d * d; } }
            __syncthreads();
            red[g * 64 + c] = m2;
            __syncthreads();
            if (tid < 64 && n0 + c < a.cout) {
                float* dst = a.part + ((size_t)rt * a.cout + (size_t)(n0 + c)) * 2;
                dst[0] = mean;
                dst[1] = ((red[c] + red[64 + c]) + red[128 + c]) + red[192 + c];
            }
        }
    }
}

// the tiles' (count, mean, centred sum of squares) -> the batch mean and biased variance of every column, in fp64 and tile order: 32 columns a workgroup,
// eight shares of the tiles each, the shares summed in share order.  The sum of squares about a tile's STORED mean m_t is exact about any pivot:
// sum (y - mean)^2 = sum (y - m_t)^2 + n_t (m_t - mean)^2 + 2 (m_t - mean) sum (y - m_t), the last term being rounding noise of the tile's own mean
__global__ __launch_bounds__(UL_BLOCK) void ul_stats_finalize_kernel(long long rows, int cout, long long row_tiles, const float* __restrict__ part, float eps,
                                                                      float momentum, float* __restrict__ moving_mean, float* __restrict__ moving_var,
                                                                      float* __restrict__ save_mean, float* __restrict__ save_invstd)
{
    __shared__ double red[8][32];
    const int cl = threadIdx.x & 31, g = threadIdx.x >> 5, c = blockIdx.x * 32 + cl;
    const bool ok = c < cout;
    double s = 0.0;
    if (ok)
        for (long long t = g; t < row_tiles; t += 8) {
            const long long left = rows - t * UL_T;
            s += (double)(left < UL_T ? left : UL_T) * (double)part[((size_t)t * cout + c) * 2];
        }
    red[g][cl] = s;
    __syncthreads();
    double mean = 0.0;
    for (int j = 0; j < 8; j++) mean += red[j][cl];
    mean /= (double)rows;
    __syncthreads();
    double m2 = 0.0;
    if (ok)
        for (long long t = g; t < row_tiles; t += 8) {
            const long long left = rows - t * UL_T;
            const double d = (double)part[((size_t)t * cout + c) * 2] - mean;
            m2 += (double)part[((size_t)t * cout + c) * 2 + 1] + (double)(left < UL_T ? left : UL_T) * d * d;
        }
    red[g][cl] = m2;
    __syncthreads();
    if (g == 0 && ok) {
        double tot = 0.0;
        for (int j = 0; j < 8; j++) tot += red[j][cl];
        // (tfbn_finish_stats' statements in this kernel's own order: written through that function the kernel compiles to another instruction order)
        const double var = tot / (double)rows;                     // biased (tf.nn.moments)
        const float fm = (float)mean, fv = (float)var;
        save_mean[c] = fm;
        save_invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
        if (moving_mean) moving_mean[c] = moving_mean[c] * momentum + fm * (1.f - momentum);
        if (moving_var) moving_var[c] = moving_var[c] * momentum + fv * (1.f - momentum);
    }
}

// ---- elementwise passes: a thread per (row, group of four columns), trips of rb rows, workgroups walking the trips past the grid cap
template <class F>
__device__ __forceinline__ void ul_walk(long long rows, int ncg, int rb, CblFastDiv dv, F f)
{
    const long long trips = (rows + rb - 1) / rb;
    for (long long t = blockIdx.x; t < trips; t += gridDim.x) {
        const long long r0 = t * rb, left = rows - r0;
        const int items = (left < rb ? (int)left : rb) * ncg;
        for (int it = threadIdx.x; it < items; it += UL_BLOCK) {
            const int r = (int)cbl_fastdiv((unsigned)it, dv);
            f(r0 + r, it - r * ncg);
        }
    }
}

struct UlWalk {
    long long rows;
    int cout, ncg, rb, vec, act, bn_mode;
    CblFastDiv dv;
    float inv_n;
    const float *y, *out_in, *go, *mean, *invstd, *gamma, *beta, *shortcut, *sums;
    float *out, *dy, *gs;
};

// bn_mode 1, second pass of the forward call: out = act(bn(y) + shortcut)
__global__ __launch_bounds__(UL_BLOCK) void ul_normalize_kernel(UlWalk a)
{
    ul_walk(a.rows, a.ncg, a.rb, a.dv, [&](long long row, int cg) {
        const int c = 4 * cg, nv = a.cout - c;
        const size_t o = (size_t)row * a.cout + c;
        const pair_f32x4 y = tfbn_ld4(a.y + o, a.vec != 0, nv);
        pair_f32x4 sc = {0.f, 0.f, 0.f, 0.f}, r = {0.f, 0.f, 0.f, 0.f};
        if (a.shortcut) sc = tfbn_ld4(a.shortcut + o, a.vec != 0, nv);
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (q < nv) r[q] = pair_act(a.act, ul_z(y[q], true, a.mean[c + q], a.invstd[c + q], a.gamma[c + q], a.beta[c + q], sc[q]));
        tfbn_st4(a.out + o, r, a.vec != 0, nv);
    });
}

// backward, second pass: dz = grad_out * act'(out) (= grad_shortcut), dy = dz through the batch norm, written once
__global__ __launch_bounds__(UL_BLOCK) void ul_dy_kernel(UlWalk a)
{
    ul_walk(a.rows, a.ncg, a.rb, a.dv, [&](long long row, int cg) {
        const int c = 4 * cg, nv = a.cout - c;
        const size_t o = (size_t)row * a.cout + c;
        pair_f32x4 dz = tfbn_ld4(a.go + o, a.vec != 0, nv), dy = {0.f, 0.f, 0.f, 0.f};
        if (a.act) {
            const pair_f32x4 h = tfbn_ld4(a.out_in + o, a.vec != 0, nv);
#pragma unroll
            for (int q = 0; q < 4; q++) dz[q] = dz[q] * pair_dact(a.act, h[q]);
        }
        if (a.gs) tfbn_st4(a.gs + o, dz, a.vec != 0, nv);
        if (!a.dy) return;
        if (a.bn_mode == 0) dy = dz;
        else {
            const pair_f32x4 y = a.bn_mode == 1 ? tfbn_ld4(a.y + o, a.vec != 0, nv) : dz;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if (q >= nv) continue;
                const float invstd = a.invstd[c + q], gi = a.gamma[c + q] * invstd;
                if (a.bn_mode == 1) {
                    const float xh = tfbn_xhat(y[q], a.mean[c + q], invstd);
                    dy[q] = gi * ((dz[q] - a.sums[c + q] * a.inv_n) - xh * (a.sums[a.cout + c + q] * a.inv_n));
                } else dy[q] = gi * dz[q];
            }
        }
        tfbn_st4(a.dy + o, dy, a.vec != 0, nv);
    });
}

struct UlSums {
    long long rows;
    int cout, act;
    const float *go, *out, *y, *mean, *invstd;
    double* part;                                                   // (gridDim.x, cout, 2)
};

// backward, first pass (bn_mode 1 and 2 only): per column sum dz and sum dz * xhat.  Thread (column, row share g of 4); a workgroup's rows are 4 blockIdx.x + g, + 4 gridDim.x, ...
__global__ __launch_bounds__(UL_BLOCK) void ul_colsum_kernel(UlSums a)
{
    __shared__ double red[2][4][64];
    const int cl = threadIdx.x & 63, g = threadIdx.x >> 6, c = blockIdx.y * 64 + cl;
    const bool ok = c < a.cout;
    double s1 = 0.0, s2 = 0.0;
    if (ok) {
        const float mean = a.mean[c], invstd = a.invstd[c];
        for (long long r = 4ll * blockIdx.x + g; r < a.rows; r += 4ll * gridDim.x) {
            const size_t o = (size_t)r * a.cout + c;
            float dz = a.go[o];
            if (a.act) dz = dz * pair_dact(a.act, a.out[o]);
            s1 += (double)dz;
            s2 += (double)(dz * tfbn_xhat(a.y[o], mean, invstd));
        }
    }
    red[0][g][cl] = s1; red[1][g][cl] = s2;
    __syncthreads();
    if (g == 0 && ok) {
        double* dst = a.part + ((size_t)blockIdx.x * a.cout + c) * 2;
        dst[0] = ((red[0][0][cl] + red[0][1][cl]) + red[0][2][cl]) + red[0][3][cl];
        dst[1] = ((red[1][0][cl] + red[1][1][cl]) + red[1][2][cl]) + red[1][3][cl];
    }
}

struct UlDgrad {
    long long rows, row_tiles;
    int cin, cout, veca, vecb;
    const float *dy, *w;
    float* gx;
};
// grad_x = dy @ weights^T: the contraction runs over c_out, both operands k-contiguous
__global__ __launch_bounds__(UL_BLOCK) void ul_dgrad_kernel(UlDgrad a)
{
    __shared__ __attribute__((aligned(16))) float As[UL_PANEL];
    __shared__ __attribute__((aligned(16))) float Bs[UL_PANEL];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, kq = lane >> 4;
    const long long n0 = (long long)blockIdx.y * UL_T;
    for (long long rt = blockIdx.x; rt < a.row_tiles; rt += gridDim.x) {
        const long long m0 = rt * UL_T;
        pair_f32x4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; t++) acc[t] = pair_f32x4{0.f, 0.f, 0.f, 0.f};
        ul_tile_product<true, true>(a.dy, a.cout, a.veca != 0, a.w, a.cout, a.vecb != 0, m0, a.rows, n0, a.cin, 0, a.cout, As, Bs, acc, [](int) {});
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const long long col = n0 + 16 * t + n;
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const long long row = m0 + 16 * wave + 4 * kq + v;
                if (row < a.rows && col < a.cin) a.gx[(size_t)row * a.cin + col] = acc[t][v];
            }
        }
    }
}

struct UlWgrad {
    long long rows, chunk_rows;
    int cin, cout, veca, vecb, tiles_n;
    const float *x, *dy;
    float *gw, *gb, *partial;                                       // partial: (chunks, cin * cout + cout) when there are several chunks; gw NULL: grad_biases alone
};
// grad_weights[ci][co] = sum_r x[r][ci] dy[r][co] over the rows of chunk blockIdx.y: the contraction runs over the rows, which are the panels' rows.  The
// workgroups of grad_weights' first row tile also sum dy's columns (fp64): grad_biases
__global__ __launch_bounds__(UL_BLOCK) void ul_wgrad_kernel(UlWgrad a)
{
    __shared__ __attribute__((aligned(16))) float As[UL_PANEL];
    __shared__ __attribute__((aligned(16))) float Bs[UL_PANEL];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, kq = lane >> 4;
    const int tm = blockIdx.x / a.tiles_n, tn = blockIdx.x - tm * a.tiles_n;
    const long long m0 = (long long)tm * UL_T, n0 = (long long)tn * UL_T;
    const long long rbeg = (long long)blockIdx.y * a.chunk_rows, rend = min(a.rows, rbeg + a.chunk_rows);
    const bool sums = tm == 0 && tid < UL_T;
    double bsum = 0.0;
    pair_f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = pair_f32x4{0.f, 0.f, 0.f, 0.f};
    ul_tile_product<false, false>(a.x, a.cin, a.veca != 0, a.dy, a.cout, a.vecb != 0, m0, a.cin, n0, a.cout, rbeg, rend, As, Bs, acc, [&](int) {
        if (sums) {
            float s = 0.f;                                          // (rows past the chunk are staged as zeros)
#pragma unroll 8
            for (int r = 0; r < UL_KP; r++) s += Bs[r * UL_LDN + tid];
            bsum += (double)s;
        }
    });
    const size_t width = (size_t)a.cin * a.cout + a.cout;
    float* gw = !a.gw ? nullptr : a.partial ? a.partial + (size_t)blockIdx.y * width : a.gw;
    float* gb = a.partial ? a.partial + (size_t)blockIdx.y * width + (size_t)a.cin * a.cout : a.gb;
    if (gw) {
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const long long col = n0 + 16 * t + n;
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const long long row = m0 + 16 * wave + 4 * kq + v;
                if (row < a.cin && col < a.cout) gw[(size_t)row * a.cout + col] = acc[t][v];
            }
        }
    }
    if (sums && gb && n0 + tid < a.cout) gb[n0 + tid] = (float)bsum;
}
// grad_weights / grad_biases = the chunks' partials summed in chunk order (fp64); plain stores
__global__ __launch_bounds__(UL_BLOCK) void ul_wgrad_combine_kernel(int cin, int cout, int nchunks, const float* __restrict__ partial, float* __restrict__ gw,
                                                                     float* __restrict__ gb)
{
    const size_t wn = (size_t)cin * cout, width = wn + cout, e = (size_t)blockIdx.x * UL_BLOCK + threadIdx.x;
    if (e >= width || (e < wn ? !gw : !gb)) return;                 // (grad_biases alone: the weights' part of the partials was never written)
    double s = 0.0;
#pragma unroll 4
    for (int j = 0; j < nchunks; j++) s += (double)partial[(size_t)j * width + e];
    if (e < wn) gw[e] = (float)s;
    else gb[e - wn] = (float)s;
}

// The plain product C (M, N) = A (M, K) @ B with its CONTRACTION split over blockIdx.z (up_conv's two products at the coarse layer's few rows, where the
// 64 x 64 tiles alone leave compute units idle): split z covers the contraction steps [z kspan, (z + 1) kspan), kspan a multiple of the panel, and stores its
// tile of partials at part[z]; ul_split_combine_kernel sums the splits in split order (fp64).  B (K, N), or B_KC: (N, K) (grad_x's layout)
constexpr int UL_SPLIT_CUS = 256, UL_MAX_SPLITS = 8, UL_SPLIT_MIN_PANELS = 4;   // the rule of ul_split_of: tiles against the device's compute units
struct UlSplit {
    long long M, row_tiles;
    int N, K, kspan, veca, vecb;
    const float *A, *B;
    float* part;                                                    // (gridDim.z, M, N)
};
template <bool B_KC>
__global__ __launch_bounds__(UL_BLOCK) void ul_split_product_kernel(UlSplit a)
{
    __shared__ __attribute__((aligned(16))) float As[UL_PANEL];
    __shared__ __attribute__((aligned(16))) float Bs[UL_PANEL];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, kq = lane >> 4;
    const long long n0 = (long long)blockIdx.y * UL_T, kbeg = (long long)blockIdx.z * a.kspan, kend = min((long long)a.K, kbeg + a.kspan);
    float* __restrict__ dst = a.part + (size_t)blockIdx.z * (size_t)a.M * a.N;
    for (long long rt = blockIdx.x; rt < a.row_tiles; rt += gridDim.x) {
        const long long m0 = rt * UL_T;
        pair_f32x4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; t++) acc[t] = pair_f32x4{0.f, 0.f, 0.f, 0.f};
        ul_tile_product<true, B_KC>(a.A, a.K, a.veca != 0, a.B, B_KC ? a.K : a.N, a.vecb != 0, m0, a.M, n0, a.N, kbeg, kend, As, Bs, acc, [](int) {});
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const long long col = n0 + 16 * t + n;
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const long long row = m0 + 16 * wave + 4 * kq + v;
                if (row < a.M && col < a.N) dst[(size_t)row * a.N + col] = acc[t][v];
            }
        }
    }
}
__global__ __launch_bounds__(UL_BLOCK) void ul_split_combine_kernel(size_t total, int splits, const float* __restrict__ part, float* __restrict__ out)
{
    for (size_t e = (size_t)blockIdx.x * UL_BLOCK + threadIdx.x; e < total; e += (size_t)gridDim.x * UL_BLOCK) {
        double s = 0.0;
#pragma unroll 4
        for (int j = 0; j < splits; j++) s += (double)part[(size_t)j * total + e];
        out[e] = (float)s;
    }
}

// ---------------------------------------------------------------- host side
struct UlPlan {
    long long row_tiles, chunk_rows;
    int nchunks, sum_blocks;
    size_t off_dy, off_part, off_sumpart, off_sums, off_wpart, bytes;   // byte offsets from the (256-byte aligned) workspace base
};
inline UlPlan ul_plan(long long rows, int cin, int cout)
{
    UlPlan p;
    p.row_tiles = (rows + UL_T - 1) / UL_T;
    const size_t width = (size_t)cin * cout + cout;
    long long nchunks = (rows + UL_CHUNK_ROWS - 1) / UL_CHUNK_ROWS;
    const long long fit = (long long)(UL_PARTIAL_FLOATS / width);
    if (nchunks > UL_MAX_CHUNKS) nchunks = UL_MAX_CHUNKS;
    if (nchunks > fit) nchunks = fit;
    if (nchunks < 1) nchunks = 1;
    p.chunk_rows = ((rows + nchunks - 1) / nchunks + UL_KP - 1) / UL_KP * UL_KP;
    if (p.chunk_rows < UL_KP) p.chunk_rows = UL_KP;
    p.nchunks = (int)((rows + p.chunk_rows - 1) / p.chunk_rows);
    if (p.nchunks < 1) p.nchunks = 1;
    const long long sb = (rows + 3) / 4;
    p.sum_blocks = (int)(sb < 1 ? 1 : sb > UL_SUM_BLOCKS ? UL_SUM_BLOCKS : sb);
    size_t o = 0;
    p.off_dy = o;      o += pair_up256((size_t)rows * cout * sizeof(float));
    p.off_part = o;    o += pair_up256((size_t)p.row_tiles * cout * 2 * sizeof(float));
    p.off_sumpart = o; o += pair_up256((size_t)p.sum_blocks * cout * 2 * sizeof(double));
    p.off_sums = o;    o += pair_up256((size_t)cout * 2 * sizeof(float));
    p.off_wpart = o;   o += p.nchunks > 1 ? pair_up256((size_t)p.nchunks * width * sizeof(float)) : 0;
    p.bytes = o + 256;                                              // the base is rounded up to 256 bytes
    return p;
}
inline bool ul_dims_ok(int cin, int cout) { return cin <= UL_MAX_C && cout <= UL_MAX_C; }
inline void ul_walk_shape(UlWalk& a, unsigned* grid)
{
    a.ncg = (a.cout + 3) / 4;
    a.rb = UL_WALK_ITEMS / a.ncg < 1 ? 1 : UL_WALK_ITEMS / a.ncg;
    a.dv = cbl_fastdiv_make((unsigned)a.ncg);
    const long long trips = (a.rows + a.rb - 1) / a.rb;
    *grid = (unsigned)(trips > UL_WALK_BLOCKS ? UL_WALK_BLOCKS : trips);
}

// the launches the unary entries and the up_conv entries share
// bn_mode 1 behind the forward product (which left y and the tiles' statistics in part): the batch statistics, then out = act(bn(y) (+ shortcut))
inline void ul_launch_bn_tail(hipStream_t st, long long rows, int c_out, long long row_tiles, const float* part, float eps, float momentum, float* moving_mean,
                              float* moving_var, float* save_mean, float* save_invstd, const float* gamma, const float* beta, int activation, const float* y,
                              const float* shortcut, float* out)
{
    hipLaunchKernelGGL(ul_stats_finalize_kernel, dim3(cbl_div_up(c_out, 32)), dim3(UL_BLOCK), 0, st, rows, c_out, row_tiles, part, eps, momentum, moving_mean, moving_var,
                       save_mean, save_invstd);
    UlWalk a = {};
    a.rows = rows; a.cout = c_out; a.act = activation; a.bn_mode = 1;
    a.vec = tfbn_vec(c_out, y, out, shortcut);
    a.y = y; a.mean = save_mean; a.invstd = save_invstd; a.gamma = gamma; a.beta = beta; a.shortcut = shortcut; a.out = out;
    unsigned g;
    ul_walk_shape(a, &g);
    hipLaunchKernelGGL(ul_normalize_kernel, dim3(g), dim3(UL_BLOCK), 0, st, a);
}
// backward: dz = grad_out * act'(out) -> grad_shortcut (optional), dz through the batch norm -> dy (optional); sums: ul_launch_colsums' (bn_mode 1)
inline void ul_launch_dy(hipStream_t st, long long rows, int c_out, int bn_mode, int activation, const float* grad_out, const float* out, const float* y,
                         const float* save_mean, const float* save_invstd, const float* gamma, const float* sums, float* dy, float* grad_shortcut)
{
    UlWalk a = {};
    a.rows = rows; a.cout = c_out; a.act = activation; a.bn_mode = bn_mode; a.inv_n = (float)(1.0 / (double)rows);
    a.dy = dy;
    a.vec = tfbn_vec(c_out, grad_out, out, y, dy, grad_shortcut);
    a.go = grad_out; a.out_in = out; a.y = y; a.mean = save_mean; a.invstd = save_invstd; a.gamma = gamma; a.sums = sums; a.gs = grad_shortcut;
    unsigned g;
    ul_walk_shape(a, &g);
    hipLaunchKernelGGL(ul_dy_kernel, dim3(g), dim3(UL_BLOCK), 0, st, a);
}
inline void ul_launch_colsums(hipStream_t st, long long rows, int c_out, int activation, const float* grad_out, const float* out, const float* y,
                              const float* save_mean, const float* save_invstd, int sum_blocks, double* part, float* sums, float* grad_beta, float* grad_gamma)
{
    UlSums s;
    s.rows = rows; s.cout = c_out; s.act = activation;
    s.go = grad_out; s.out = out; s.y = y; s.mean = save_mean; s.invstd = save_invstd;
    s.part = part;
    hipLaunchKernelGGL(ul_colsum_kernel, dim3(sum_blocks, cbl_div_up(c_out, 64)), dim3(UL_BLOCK), 0, st, s);
    tfbn_launch_sums_finalize(st, c_out, sum_blocks, s.part, sums, grad_beta, grad_gamma);
}
inline void ul_launch_dgrad(hipStream_t st, long long rows, int c_in, int c_out, const float* dy, const float* weights, float* grad_x)
{
    UlDgrad d;
    d.rows = rows; d.row_tiles = (rows + UL_T - 1) / UL_T; d.cin = c_in; d.cout = c_out; d.veca = tfbn_vec(c_out, dy); d.vecb = tfbn_vec(c_out, weights);
    d.dy = dy; d.w = weights; d.gx = grad_x;
    const dim3 grid((unsigned)(d.row_tiles > UL_ROW_BLOCKS ? UL_ROW_BLOCKS : d.row_tiles), cbl_div_up(c_in, UL_T));
    hipLaunchKernelGGL(ul_dgrad_kernel, grid, dim3(UL_BLOCK), 0, st, d);
}
// grad_weights (c_in, c_out) and / or grad_biases of x (rows, c_in) and dy (rows, c_out); p = ul_plan(rows, c_in, c_out), wpart its partials (nchunks > 1)
inline void ul_launch_wgrad(hipStream_t st, const UlPlan& p, long long rows, int c_in, int c_out, const float* x, const float* dy, float* grad_weights,
                            float* grad_biases, float* wpart)
{
    UlWgrad w;
    w.rows = rows; w.chunk_rows = p.chunk_rows; w.cin = c_in; w.cout = c_out; w.veca = tfbn_vec(c_in, x); w.vecb = tfbn_vec(c_out, dy);
    w.tiles_n = (int)cbl_div_up(c_out, UL_T);
    w.x = x; w.dy = dy; w.gw = grad_weights; w.gb = grad_biases;
    w.partial = p.nchunks > 1 ? wpart : nullptr;
    // grad_biases alone: only the first row of tiles, the one that sums dy's columns (its own product is not stored)
    const unsigned tiles_m = grad_weights ? cbl_div_up(c_in, UL_T) : 1u;
    hipLaunchKernelGGL(ul_wgrad_kernel, dim3(tiles_m * w.tiles_n, p.nchunks), dim3(UL_BLOCK), 0, st, w);
    if (p.nchunks > 1)
        hipLaunchKernelGGL(ul_wgrad_combine_kernel, dim3(cbl_div_up((long long)c_in * c_out + c_out, UL_BLOCK)), dim3(UL_BLOCK), 0, st, c_in, c_out, p.nchunks,
                           w.partial, grad_weights, grad_biases);
}

}  // namespace

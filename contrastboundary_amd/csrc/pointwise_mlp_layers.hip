// a14: PointWiseMLP with fc_num 2 and 3 — per-pair layers, each with its own batch norm over all n*K pair rows.
// tensorflow/models/local_aggregation_operators.py:589-600 (batch_conv1d_1x1, basic_operators.py:243-289; batch norm :134-152): fc_0 .. fc_{fc_num-2} of width
// H = max(in_fdim / 2, 9), then fc_{fc_num} of width C_out; no layer has a bias, every layer has a batch norm and the activation.  L = fc_num - 1, N = n K,
// for the pair (i, k), j = idx[i, k]:
//     y_0 = ((s_j - q_i) / radius) . W_p + Cen[idx[i,0]] + Nbr[j]                                     the fold of pointwise_mlp.hip, width H
//     xh_l = (y_l - mean_l) * invstd_l    z_l = gamma_l * xh_l + beta_l    h_l = act(z_l)             l = 0 .. L
//     y_{l+1} = h_l @ W_{l+1}                                                                         W_1 (H, H) when L = 2, W_L (H, C_out)
//     out[i] = reduce_k mask[i,k] * h_L                                                               sum | mean (:609-613) | max (a shadow pair counts as 0)
// Shadow pairs go through every layer and every statistic; only the final mask removes them.
//
// MI355X mapping.  A workgroup of four waves takes a tile of whole queries per trip: R = their pair rows padded to a multiple of 16, H zero-padded to HP = a
// multiple of 16 inside the kernel.  The row convention, the y_0 fold, the MFMA product and weight-gradient tiles, the target-side chunk walk and the
// host-side tile planning are pair_tile.h's, shared with adaptive_weight_mlp.hip.  LDS holds xh_l of the hidden layers (L buffers R x LDH), one column tile
// of the last layer (R x CT, CT = 16 / 32 / 64 columns: the (R, C_out) product is never held whole) and, in the backward passes, one R x LDH gradient buffer.
//   layers   : a pair recomputes to the same bits in every sweep and on the target side, which 'max' relies on; the A operand is h_l = act(gamma xh + beta)
//              formed from the stored xh at the load, gamma = beta = 0 in the padded columns, so these stay exactly zero whatever beta is; the weights are
//              the B operand from global memory (L1 / L2 resident)
//   sums     : per column over the tile's REAL rows (rowI >= 0; padding rows and padded columns enter no statistic), fp64 per thread, combined through LDS in a
//              fixed order and added to the workgroup's own fp64 partial in the workspace; finalize kernels add the partials in workgroup order (fp64)
// With batch statistics layer l + 1 cannot be formed before the statistics of layer l are final:
//   forward   L + 2 sweeps of ONE kernel (`upto` = the layer whose sum y, sum y^2 the sweep takes; the last sweep normalises, activates, masks, reduces),
//             a finalize kernel behind each statistics sweep (mean, invstd, the TF update of the moving statistics).  bn_mode 0 / 2: the last sweep alone.
//   backward  BQ by query, L + 2 sweeps of one kernel: sweep s = 0 .. L stops at layer lo = L - s and takes sum dz_lo, sum dz_lo xh_lo (= d beta, d gamma),
//             the last one forms dy_0: grad_center, partial sums of grad_w_pos.  A sweep that has dy_l adds h_{l-1}^T dy_l (MFMA, the pairs are the
//             contraction) to the workgroup's fp32 partial of grad_hidden_w.  'max': the first sweep counts the ties against the forward's `out`.
//             bn_mode 0 / 2: one sweep.  BT by target over the transposed table: chunks of R pairs walk forward and back to dy_0 with every sum final.
// No float atomics; every output is stored once in a fixed order.  LDS: one of three static sizes (32 / 64 / 120 KB of rows + 21 KB of row data, layer
// constants and the reduction scratch) of gfx950's 160 KB.
#include "pair_tile.h"

namespace {

enum { PLM_BN_NONE = 0, PLM_BN_BATCH = 1, PLM_BN_MOVING = 2 };
constexpr int PLM_YCT = 4, PLM_LAYW = 160;
constexpr int PLM_HMIN = 16, PLM_HMAX = 144, PLM_KMAX = 128, PLM_KWIDE = 48, PLM_HNARROW = 64, PLM_CMAX = 1024;
// grid caps (two workgroups per compute unit; a trip is a chain of phases behind barriers); BQ's also bounds the fp32 weight partials: at most
// PAIR_BQ_PARTIAL floats of them, never fewer than PLM_BQ_BLOCKS_MIN workgroups
constexpr int PLM_F_BLOCKS = 512, PLM_BQ_BLOCKS = 512, PLM_BQ_BLOCKS_MIN = 64, PLM_BT_BLOCKS = 512;
constexpr int PLM_LDS0 = 8192, PLM_LDS1 = 16384, PLM_LDS2 = 30720;                                 // floats of row buffers

struct PlmArgs {
    int n, n0, K, H, HP, LDH, nct, C, L, WT, act, bn, red;
    int R, tq, tpt, CT, LDY, nbuf;              // rows of a tile, queries / targets of a trip, columns of a last-layer tile and its row pitch, R x LDH buffers
    const float* q; const float* s; const int* idx;
    const float* cen; const float* nbr; const float* wp; const float* hw;
    const float* gamma; const float* beta; const float* mean; const float* invstd;                 // packed: layer l < L at l H, the last layer at L H
    float inv_radius;
    const int* padding_num;
};
struct PlmBwd {
    const float* go; const float* out; const float* coef;            // coef: [sum dz / N | sum dz xh / N], packed like gamma
    float* inv_nn; float* ties;
};
// what a walk emits: lo = the layer it stops at (-1: down to dy_0); sums: this workgroup's fp64 partial [WT sum dz | WT sum dz xh | 3 H dp^T dy_0];
// wsum: its fp32 partial of grad_hidden_w; first: the workgroup's first trip (stores) or a later one (adds)
struct PlmEmit { int lo; bool ties; double* sums; float* wsum; bool first; };
struct PlmLds { float* buf; float* dp; int* rowI; int* rowJ; int* rowC; float* cnt; float* lay; double* red; };
// the last layer's constants of one column
struct PlmCol { float mu, is, ga, be, k0, k1; };

#define PLM_LDS_DECL(L)                                                                                                                  \
    __shared__ float plm_buf[LDSF]; __shared__ float plm_dp[PAIR_RMAX * 3]; __shared__ int plm_ri[PAIR_RMAX]; __shared__ int plm_rj[PAIR_RMAX];   \
    __shared__ int plm_rc[PAIR_RMAX]; __shared__ float plm_cnt[PAIR_RMAX]; __shared__ float plm_lay[2 * 6 * PLM_LAYW];                    \
    __shared__ double plm_red[3 * PAIR_BLOCK];                                                                                           \
    PlmLds L; L.buf = plm_buf; L.dp = plm_dp; L.rowI = plm_ri; L.rowJ = plm_rj; L.rowC = plm_rc; L.cnt = plm_cnt; L.lay = plm_lay; L.red = plm_red

// the constants of hidden layer l at column k: 0 mean, 1 invstd, 2 gamma, 3 beta, 4 sum dz / N, 5 sum dz xh / N — all zero in the padded columns
__device__ __forceinline__ float plm_lay(const PlmLds& L, int l, int which, int k) { return L.lay[(l * 6 + which) * PLM_LAYW + k]; }
// h_l from the stored xh_l (exactly 0 in a padded column: gamma = beta = 0 there)
__device__ __forceinline__ float plm_h(const PlmArgs& a, const PlmLds& L, int l, float xh, int k)
{
    return pair_act(a.act, plm_lay(L, l, 2, k) * xh + plm_lay(L, l, 3, k));
}
// gradient at y through the batch norm from the gradient at z
__device__ __forceinline__ float plm_bn_back(int bn, float ga, float is, float k0, float k1, float dz, float xh)
{
    if (bn == PLM_BN_BATCH) return (ga * is) * ((dz - k0) - xh * k1);
    if (bn == PLM_BN_MOVING) return (ga * is) * dz;
    return dz;
}

__device__ __forceinline__ void plm_load_layers(const PlmArgs& a, const PlmLds& L, const float* coef)
{
    for (int it = threadIdx.x; it < 2 * PLM_LAYW; it += PAIR_BLOCK) {
        const int l = it / PLM_LAYW, k = it - l * PLM_LAYW;
        const bool live = l < a.L && k < a.H, bn = a.bn != PLM_BN_NONE;
        const int at = l * a.H + k;
        float* d = L.lay + (size_t)l * 6 * PLM_LAYW + k;
        d[0] = (live && bn) ? a.mean[at] : 0.f;
        d[PLM_LAYW] = live ? (bn ? a.invstd[at] : 1.f) : 0.f;
        d[2 * PLM_LAYW] = live ? ((bn && a.gamma) ? a.gamma[at] : 1.f) : 0.f;
        d[3 * PLM_LAYW] = (live && bn && a.beta) ? a.beta[at] : 0.f;
        const bool cf = live && coef && a.bn == PLM_BN_BATCH;
        d[4 * PLM_LAYW] = cf ? coef[at] : 0.f;
        d[5 * PLM_LAYW] = cf ? coef[a.WT + at] : 0.f;
    }
}
__device__ __forceinline__ PlmCol plm_col(const PlmArgs& a, const float* coef, int cc)
{
    PlmCol t;
    const bool live = cc < a.C, bn = a.bn != PLM_BN_NONE;
    const int at = a.L * a.H + (live ? cc : 0);
    t.mu = (live && bn) ? a.mean[at] : 0.f;
    t.is = (live && bn) ? a.invstd[at] : 1.f;
    t.ga = (live && bn && a.gamma) ? a.gamma[at] : 1.f;
    t.be = (live && bn && a.beta) ? a.beta[at] : 0.f;
    const bool cf = live && coef && a.bn == PLM_BN_BATCH;
    t.k0 = cf ? coef[at] : 0.f;
    t.k1 = cf ? coef[a.WT + at] : 0.f;
    return t;
}

// fc_0: X[r][m] = xh_0 (raw: y_0 itself, for the statistics sweep)
__device__ __forceinline__ void plm_first(const PlmArgs& a, const PlmLds& L, float* __restrict__ X, bool raw)
{
    pair_fold_rows(a, L, a.H, a.HP, a.wp, a.cen, a.nbr, X, a.LDH,
                   [&](int m, float y0) { return raw ? y0 : (y0 - plm_lay(L, 0, 0, m)) * plm_lay(L, 0, 1, m); });
}

// fc_1 of fc_num 3: X1 = xh_1 (raw: y_1) from xh_0
__device__ __forceinline__ void plm_hidden(const PlmArgs& a, const PlmLds& L, const float* X0, float* X1, bool raw)
{
    const float* __restrict__ W = a.hw;
    pair_mfma<PAIR_NCT>(a.R, a.HP, a.nct,
        [&](int r, int k) { return plm_h(a, L, 0, X0[r * a.LDH + k], k); },
        [&](int k, int c) { return (k < a.H && c < a.H) ? W[(size_t)k * a.H + c] : 0.f; },
        [&](int, int) { return 0.f; },
        [&](int r, int c, float y) { X1[r * a.LDH + c] = c < a.H ? (raw ? y : (y - plm_lay(L, 1, 0, c)) * plm_lay(L, 1, 1, c)) : 0.f; });
}
// the last layer's columns c0 .. c0 + CT: Y = y_L (raw) from xh_{L-1}
__device__ __forceinline__ void plm_last(const PlmArgs& a, const PlmLds& L, const float* X, float* Y, int c0)
{
    const float* __restrict__ W = a.hw + (a.L == 2 ? (size_t)a.H * a.H : 0);
    const int l = a.L - 1;
    pair_mfma<PLM_YCT>(a.R, a.HP, a.CT / 16,
        [&](int r, int k) { return plm_h(a, L, l, X[r * a.LDH + k], k); },
        [&](int k, int c) { return (k < a.H && c0 + c < a.C) ? W[(size_t)k * a.C + c0 + c] : 0.f; },
        [&](int, int) { return 0.f; },
        [&](int r, int c, float y) { Y[r * a.LDY + c] = y; });
}

// dst[v * stride + c] (+)= sum over the tile's real rows of f(r, c)[v], c < width <= 256: thread (slice, column) takes every nsl-th row in fp64, the slices
// are added in their order.  Starts behind a barrier, ends behind one.
template <int V, class F>
__device__ __forceinline__ void plm_colsum(const PlmLds& L, int R, int width, bool first, double* __restrict__ dst, size_t stride, F f)
{
    const int nsl = PAIR_BLOCK / width, sl = threadIdx.x / width, c = threadIdx.x - sl * width;
    if (sl < nsl) {
        double s[V];
#pragma unroll
        for (int v = 0; v < V; v++) s[v] = 0.0;
        for (int r = sl; r < R; r += nsl) {
            if (L.rowI[r] < 0) continue;
            double t[V];
            f(r, c, t);
#pragma unroll
            for (int v = 0; v < V; v++) s[v] += t[v];
        }
#pragma unroll
        for (int v = 0; v < V; v++) L.red[v * PAIR_BLOCK + threadIdx.x] = s[v];
    }
    __syncthreads();
    if (sl == 0) {
#pragma unroll
        for (int v = 0; v < V; v++) {
            double t = 0.0;
            for (int j = 0; j < nsl; j++) t += L.red[v * PAIR_BLOCK + j * width + c];
            double* d = dst + (size_t)v * stride + c;
            *d = first ? t : *d + t;
        }
    }
    __syncthreads();
}

// ---------------------------------------------------------------- forward
// upto = the layer whose sum y, sum y^2 this sweep takes (the layers below it have their statistics); upto = L + 1: normalise, activate, mask, reduce -> out.
// partial: [WT sum y | WT sum y^2] per workgroup (PD doubles apart)
template <int LDSF>
__global__ __launch_bounds__(PAIR_BLOCK) void plm_forward_kernel(PlmArgs a, int upto, double* __restrict__ partial, size_t PD, float* __restrict__ out)
{
    PLM_LDS_DECL(L);
    const int pad = (a.red == PAIR_MEAN) ? *a.padding_num : 0;
    const int ntrips = (a.n + a.tq - 1) / a.tq;
    float* X0 = L.buf;
    float* X1 = L.buf + (size_t)a.R * a.LDH;
    float* Y = L.buf + (size_t)a.nbuf * a.R * a.LDH;
    double* mine = partial ? partial + (size_t)blockIdx.x * PD : nullptr;
    auto square = [](float y, double (&t)[2]) { t[0] = (double)y; t[1] = (double)y * (double)y; };
    plm_load_layers(a, L, nullptr);
    for (int trip = blockIdx.x; trip < ntrips; trip += gridDim.x) {
        const int i0 = trip * a.tq;
        const bool first = trip == (int)blockIdx.x;
        pair_rows_query(a, L, i0, pad);
        __syncthreads();
        plm_first(a, L, X0, upto == 0);
        __syncthreads();
        if (upto == 0) {
            plm_colsum<2>(L, a.R, a.H, first, mine, (size_t)a.WT, [&](int r, int c, double (&t)[2]) { square(X0[r * a.LDH + c], t); });
            continue;
        }
        const float* X = X0;
        if (a.L == 2) {
            plm_hidden(a, L, X0, X1, upto == 1);
            __syncthreads();
            X = X1;
            if (upto == 1) {
                plm_colsum<2>(L, a.R, a.H, first, mine + a.H, (size_t)a.WT, [&](int r, int c, double (&t)[2]) { square(X1[r * a.LDH + c], t); });
                continue;
            }
        }
        for (int c0 = 0; c0 < a.C; c0 += a.CT) {
            const int cw = min(a.CT, a.C - c0);
            plm_last(a, L, X, Y, c0);
            __syncthreads();
            if (upto == a.L) {
                plm_colsum<2>(L, a.R, cw, first, mine + a.L * a.H + c0, (size_t)a.WT, [&](int r, int c, double (&t)[2]) { square(Y[r * a.LDY + c], t); });
                continue;
            }
            for (int it = threadIdx.x; it < a.tq * cw; it += PAIR_BLOCK) {
                const int qi = it / cw, c = it - qi * cw, i = i0 + qi;
                if (i >= a.n) continue;
                const PlmCol t = plm_col(a, nullptr, c0 + c);
                float acc = a.red == PAIR_MAX ? -INFINITY : 0.f;
                for (int k = 0; k < a.K; k++) {
                    const int r = qi * a.K + k;
                    const float xh = (Y[r * a.LDY + c] - t.mu) * t.is, z = t.ga * xh + t.be;
                    const float av = pair_real(L.rowJ[r], a.n0) ? pair_act(a.act, z) : 0.f;          // activation * mask (:601): a shadow pair is 0, also under 'max'
                    if (a.red == PAIR_MAX) acc = av > acc ? av : acc; else acc += av;
                }
                if (a.red == PAIR_MEAN) acc = acc / (L.cnt[qi] + 1e-5f);                              // :609-613
                out[(size_t)i * a.C + c0 + c] = acc;
            }
            __syncthreads();
        }
    }
}

// mean, invstd and the TF update of the moving statistics of the columns off .. off + width (fp64 over the workgroups' partials in their order)
__global__ __launch_bounds__(256) void plm_fin_stats_kernel(int off, int width, int WT, int nblocks, size_t PD, const double* __restrict__ partial, double N, float eps,
                                                            float momentum, float* __restrict__ moving_mean, float* __restrict__ moving_var,
                                                            float* __restrict__ save_mean, float* __restrict__ save_invstd)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= width) return;
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
    for (int b = 0; b < nblocks; b++) { s0 += partial[(size_t)b * PD + off + c]; s1 += partial[(size_t)b * PD + WT + off + c]; }
    const double mu = s0 / N;
    double var = s1 / N - mu * mu;                                    // biased, as tf.nn.moments
    if (var < 0.0) var = 0.0;
    save_mean[off + c] = (float)mu;
    save_invstd[off + c] = (float)(1.0 / sqrt(var + (double)eps));
    // tf.layers.batch_normalization: moving = moving * momentum + batch * (1 - momentum), with the BIASED variance
    if (moving_mean) moving_mean[off + c] = moving_mean[off + c] * momentum + (float)mu * (1.f - momentum);
    if (moving_var) moving_var[off + c] = moving_var[off + c] * momentum + (float)var * (1.f - momentum);
}
// bn_mode 2: the statistics are the moving ones
__global__ __launch_bounds__(256) void plm_moving_kernel(int WT, const float* __restrict__ moving_mean, const float* __restrict__ moving_var, float eps,
                                                         float* __restrict__ mean, float* __restrict__ invstd)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < WT) { mean[c] = moving_mean[c]; invstd[c] = (float)(1.0 / sqrt((double)moving_var[c] + (double)eps)); }
}

// ---------------------------------------------------------------- backward: the walk both sides share
// rows in LDS (behind a barrier) -> forward chain, then back from the last layer to layer em.lo (-1: dy_0 in the gradient buffer, handed to tail)
template <class TAIL>
__device__ __forceinline__ void plm_walk(const PlmArgs& a, const PlmBwd& b, const PlmLds& L, const PlmEmit& em, int i0, TAIL tail)
{
    float* X0 = L.buf;
    float* X1 = L.buf + (size_t)a.R * a.LDH;
    float* DH = L.buf + (size_t)a.L * a.R * a.LDH;
    float* Y = L.buf + (size_t)a.nbuf * a.R * a.LDH;
    const bool batch = a.bn == PLM_BN_BATCH;
    auto sums = [&](int l) { return em.sums && (batch ? l == em.lo : a.bn == PLM_BN_MOVING); };
    auto wgrad = [&](int l) { return em.wsum && (batch ? l == em.lo + 1 : true); };
    plm_first(a, L, X0, false);
    __syncthreads();
    const float* XL = X0;
    if (a.L == 2) {
        plm_hidden(a, L, X0, X1, false);
        __syncthreads();
        XL = X1;
    }
    const float* __restrict__ WL = a.hw + (a.L == 2 ? (size_t)a.H * a.H : 0);
    float* wsumL = em.wsum ? em.wsum + (a.L == 2 ? (size_t)a.H * a.H : 0) : nullptr;
    for (int c0 = 0; c0 < a.C; c0 += a.CT) {
        const int cw = min(a.CT, a.C - c0);
        plm_last(a, L, XL, Y, c0);
        __syncthreads();
        if (em.ties && a.red == PAIR_MAX) {                               // how many pairs attain each maximum (shadow pairs, value 0, count)
            for (int it = threadIdx.x; it < a.tq * cw; it += PAIR_BLOCK) {
                const int qi = it / cw, c = it - qi * cw, i = i0 + qi;
                if (i >= a.n) continue;
                const PlmCol t = plm_col(a, nullptr, c0 + c);
                const float m = b.out[(size_t)i * a.C + c0 + c];
                float tc = 0.f;
                for (int k = 0; k < a.K; k++) {
                    const int r = qi * a.K + k;
                    const float xh = (Y[r * a.LDY + c] - t.mu) * t.is, z = t.ga * xh + t.be;
                    tc += ((pair_real(L.rowJ[r], a.n0) ? pair_act(a.act, z) : 0.f) == m) ? 1.f : 0.f;
                }
                b.ties[(size_t)i * a.C + c0 + c] = tc;
            }
            __syncthreads();
        }
        // dz_L of (row r, column c) from the raw y_L in Y: the reduction, the mask, the activation
        auto dzL = [&](const PlmCol& t, int r, int c, float& xh) -> float {
            const int i = L.rowI[r];
            xh = (Y[r * a.LDY + c] - t.mu) * t.is;
            const float z = t.ga * xh + t.be;
            if (i < 0 || !pair_real(L.rowJ[r], a.n0)) return 0.f;         // the mask sits behind the activation (:601): a shadow pair passes nothing on
            const size_t at = (size_t)i * a.C + c0 + c;
            const float g = b.go[at];
            float gf;
            if (a.red == PAIR_MAX) {
                const float tc = b.ties[at];
                gf = (pair_act(a.act, z) == b.out[at] && tc > 0.f) ? g / tc : 0.f;
            } else gf = g * b.inv_nn[i];
            return pair_dact(a.act, z) * gf;
        };
        if (sums(a.L)) {
            const PlmCol t = plm_col(a, nullptr, c0 + (int)threadIdx.x % cw);     // (plm_colsum's own column of this thread)
            plm_colsum<2>(L, a.R, cw, em.first, em.sums + a.L * a.H + c0, (size_t)a.WT, [&](int r, int cc, double (&v)[2]) {
                float xh;
                const float dz = dzL(t, r, cc, xh);
                v[0] = (double)dz; v[1] = (double)dz * (double)xh;
            });
        }
        if (em.lo == a.L) continue;
        {                                                                // Y <- dy_L, zero on the padding rows and behind the last column (256 % CT == 0:
            const int c = threadIdx.x % a.CT;                            //  a thread keeps its column)
            const PlmCol t = plm_col(a, b.coef, c0 + c);
            for (int r = threadIdx.x / a.CT; r < a.R; r += PAIR_BLOCK / a.CT) {
                float v = 0.f;
                if (L.rowI[r] >= 0 && c < cw) {
                    float xh;
                    const float dz = dzL(t, r, c, xh);
                    v = plm_bn_back(a.bn, t.ga, t.is, t.k0, t.k1, dz, xh);
                }
                Y[r * a.LDY + c] = v;
            }
        }
        __syncthreads();
        if (wgrad(a.L))
            pair_wgrad(a.R, a.nct, a.H, [&](int r, int p) { return plm_h(a, L, a.L - 1, XL[r * a.LDH + p], p); }, Y, a.LDY, a.CT / 16, cw, wsumL, a.C, c0,
                       em.first);
        // dh_{L-1} (+)= dy_L @ W_L[:, c0 ..]^T
        pair_mfma<PAIR_NCT>(a.R, a.CT, a.nct,
            [&](int r, int k) { return Y[r * a.LDY + k]; },
            [&](int k, int c) { return (k < cw && c < a.H) ? WL[(size_t)c * a.C + c0 + k] : 0.f; },
            [&](int r, int c) { return c0 > 0 ? DH[r * a.LDH + c] : 0.f; },
            [&](int r, int c, float v) { DH[r * a.LDH + c] = v; });
        __syncthreads();
    }
    if (em.lo == a.L) return;
    for (int l = a.L - 1; l >= 0; l--) {
        const float* X = l == 0 ? X0 : X1;
        // dz_l = dh_l act'(z_l): every valid row (a shadow pair is a pair like any other below the final mask)
        auto dzl = [&](int r, int m, float& xh) -> float {
            xh = X[r * a.LDH + m];
            return DH[r * a.LDH + m] * pair_dact(a.act, plm_lay(L, l, 2, m) * xh + plm_lay(L, l, 3, m));
        };
        if (sums(l))
            plm_colsum<2>(L, a.R, a.H, em.first, em.sums + l * a.H, (size_t)a.WT, [&](int r, int m, double (&v)[2]) {
                float xh;
                const float dz = dzl(r, m, xh);
                v[0] = (double)dz; v[1] = (double)dz * (double)xh;
            });
        if (em.lo == l) return;
        for (int it = threadIdx.x; it < a.R * a.HP; it += PAIR_BLOCK) {   // dh_l -> dy_l in place
            const int r = it / a.HP, m = it - r * a.HP;
            float v = 0.f;
            if (L.rowI[r] >= 0 && m < a.H) {
                float xh;
                const float dz = dzl(r, m, xh);
                v = plm_bn_back(a.bn, plm_lay(L, l, 2, m), plm_lay(L, l, 1, m), plm_lay(L, l, 4, m), plm_lay(L, l, 5, m), dz, xh);
            }
            DH[r * a.LDH + m] = v;
        }
        __syncthreads();
        if (l >= 1) {
            if (wgrad(l)) {
                pair_wgrad(a.R, a.nct, a.H, [&](int r, int p) { return plm_h(a, L, l - 1, X0[r * a.LDH + p], p); }, DH, a.LDH, a.nct, a.H, em.wsum, a.H, 0,
                           em.first);
                __syncthreads();
            }
            const float* __restrict__ W = a.hw;                          // dh_{l-1} = dy_l @ W_l^T, in place
            pair_mfma<PAIR_NCT>(a.R, a.HP, a.nct,
                [&](int r, int k) { return DH[r * a.LDH + k]; },
                [&](int k, int c) { return (k < a.H && c < a.H) ? W[(size_t)c * a.H + k] : 0.f; },
                [&](int, int) { return 0.f; },
                [&](int r, int c, float v) { DH[r * a.LDH + c] = v; });
            __syncthreads();
        }
    }
    tail(DH);
}

// ---------------------------------------------------------------- BQ
template <int LDSF>
__global__ __launch_bounds__(PAIR_BLOCK) void plm_bwd_query_kernel(PlmArgs a, PlmBwd b, int lo, int first_sweep, double* __restrict__ partial, size_t PD,
                                                                  float* __restrict__ wpartial, size_t PW, float* __restrict__ grad_center, int wpos)
{
    PLM_LDS_DECL(L);
    const int pad = (a.red == PAIR_MEAN) ? *a.padding_num : 0;
    const int ntrips = (a.n + a.tq - 1) / a.tq;
    PlmEmit em;
    em.lo = lo; em.ties = first_sweep != 0;
    em.sums = partial + (size_t)blockIdx.x * PD;
    em.wsum = wpartial ? wpartial + (size_t)blockIdx.x * PW : nullptr;
    plm_load_layers(a, L, b.coef);
    for (int trip = blockIdx.x; trip < ntrips; trip += gridDim.x) {
        const int i0 = trip * a.tq;
        em.first = trip == (int)blockIdx.x;
        pair_rows_query(a, L, i0, pad);
        __syncthreads();
        if (first_sweep)
            for (int qi = threadIdx.x; qi < a.tq; qi += PAIR_BLOCK)
                if (i0 + qi < a.n) b.inv_nn[i0 + qi] = a.red == PAIR_MEAN ? 1.0f / (L.cnt[qi] + 1e-5f) : 1.0f;
        __syncthreads();
        plm_walk(a, b, L, em, i0, [&](const float* DY) {
            if (grad_center) {
                for (int it = threadIdx.x; it < a.tq * a.H; it += PAIR_BLOCK) {
                    const int qi = it / a.H, m = it - qi * a.H, i = i0 + qi;
                    if (i >= a.n) continue;
                    float s = 0.f;
                    for (int k = 0; k < a.K; k++) s += DY[(qi * a.K + k) * a.LDH + m];
                    grad_center[(size_t)i * a.H + m] = s;
                }
            }
            if (wpos)
                plm_colsum<3>(L, a.R, a.H, em.first, em.sums + 2 * (size_t)a.WT, (size_t)a.H, [&](int r, int m, double (&v)[3]) {
                    const double dy = (double)DY[r * a.LDH + m];
                    v[0] = (double)L.dp[3 * r] * dy; v[1] = (double)L.dp[3 * r + 1] * dy; v[2] = (double)L.dp[3 * r + 2] * dy;
                });
        });
        __syncthreads();
    }
}

// grad_beta = sum dz, grad_gamma = sum dz xh and the two coefficients of the batch-norm backward, columns off .. off + width
__global__ __launch_bounds__(256) void plm_fin_bn_kernel(int off, int width, int WT, int nblocks, size_t PD, const double* __restrict__ partial, double N,
                                                         float* __restrict__ grad_gamma, float* __restrict__ grad_beta, float* __restrict__ coef)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= width) return;
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
    for (int b = 0; b < nblocks; b++) { s0 += partial[(size_t)b * PD + off + c]; s1 += partial[(size_t)b * PD + WT + off + c]; }
    if (grad_gamma) grad_gamma[off + c] = (float)s1;
    if (grad_beta) grad_beta[off + c] = (float)s0;
    coef[off + c] = (float)(s0 / N); coef[WT + off + c] = (float)(s1 / N);
}
// grad_hidden_w (PW floats) from the fp32 partials, grad_w_pos (3 H) from the fp64 ones, added in the order of the workgroups in fp64
__global__ __launch_bounds__(256) void plm_fin_w_kernel(int H, int WT, int nblocks, size_t PW, size_t PD, const float* __restrict__ wpartial,
                                                        const double* __restrict__ partial, float* __restrict__ grad_hw, float* __restrict__ grad_w_pos)
{
    const size_t total = PW + 3 * (size_t)H;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        double s = 0.0;
        if (e < PW) {
            if (!grad_hw) continue;
#pragma unroll 4
            for (int bk = 0; bk < nblocks; bk++) s += (double)wpartial[(size_t)bk * PW + e];
            grad_hw[e] = (float)s;
        } else {
            if (!grad_w_pos) continue;
#pragma unroll 4
            for (int bk = 0; bk < nblocks; bk++) s += partial[(size_t)bk * PD + 2 * (size_t)WT + (e - PW)];
            grad_w_pos[e - PW] = (float)s;
        }
    }
}

// ---------------------------------------------------------------- BT
template <int LDSF>
__global__ __launch_bounds__(PAIR_BLOCK) void plm_bwd_target_kernel(PlmArgs a, PlmBwd b, CblFastDiv dvK, const int* __restrict__ order,
                                                                   const int* __restrict__ inv_start, const int* __restrict__ inv_src,
                                                                   float* __restrict__ grad_neighbor)
{
    PLM_LDS_DECL(L);
    const int ntrips = (a.n0 + a.tpt - 1) / a.tpt;
    PlmEmit em;
    em.lo = -1; em.ties = false; em.sums = nullptr; em.wsum = nullptr; em.first = false;
    plm_load_layers(a, L, b.coef);
    for (int trip = blockIdx.x; trip < ntrips; trip += gridDim.x) {
        const int t_lo = trip * a.tpt, t_hi = min(t_lo + a.tpt, a.n0);
        const int e_lo = inv_start[t_lo], e_hi = inv_start[t_hi];
        int ce = e_lo;
        do {                                                             // chunks of R pairs; at least one, so that a target without pairs is stored too
            const bool last = ce + a.R >= e_hi;
            pair_rows_target(a, L, dvK, inv_src, ce, e_hi);
            __syncthreads();
            plm_walk(a, b, L, em, 0, [&](const float* DY) {                     // grad_neighbor[j, m] = sum over j's pairs of dy_0
                pair_target_sum(a, a.H, DY, a.LDH, t_lo, t_hi, ce, last, order, inv_start, grad_neighbor);
            });
            __syncthreads();
            ce += a.R;
        } while (ce < e_hi);
    }
}

// ---------------------------------------------------------------- host side
int plm_check(int n, int n0, int K, int H, int C, int layers, float radius, int bn_mode, int activation, int reduction)
{
    if (n < 0 || n0 < 0 || K <= 0 || H <= 0 || C <= 0 || layers < 0 || !(radius > 0.f)) return CBL_ERR_BAD_ARG;
    if (bn_mode < 0 || bn_mode > PLM_BN_MOVING || activation < 0 || activation > 2 || reduction < 0 || reduction > PAIR_MAX) return CBL_ERR_BAD_ARG;
    if (layers < 1 || layers > 2 || K > PLM_KMAX || C % 4 != 0 || C > PLM_CMAX) return CBL_ERR_UNSUPPORTED;
    if (H < PLM_HMIN || H > PLM_HMAX || (K > PLM_KWIDE && H > PLM_HNARROW)) return CBL_ERR_UNSUPPORTED;
    return CBL_OK;
}

// the plan of pair_plan_query / pair_plan_target — the LDS size (0, 1, 2), the row pitch, the last layer's tile width and the rows of a tile — for `nbuf`
// R x LDH buffers + one R x (CT + 4): the smallest size that holds `want` rows, else the smallest that holds `need`; at each size rows HP + 4 floats apart
// and 64 columns where that fits, HP and 32 where not.  The callable writes what it chose into a.nbuf, a.LDH, a.CT, a.LDY: use it within the expression
// that makes it, on the args object that is launched
inline auto plm_plan(PlmArgs& a, int nbuf)
{
    return [&a, nbuf](int need, int want, int* rows) {
        const int sizes[3] = {PLM_LDS0, PLM_LDS1, PLM_LDS2};
        const int ct = a.C <= 16 ? 16 : a.C <= 32 ? 32 : 64;
        a.nbuf = nbuf;
        for (int pass = 0; pass < 2; pass++)
            for (int z = 0; z < 3; z++)
                for (int tight = 0; tight < 2; tight++) {
                    a.LDH = a.HP + (tight ? 0 : 4);
                    a.CT = (tight && ct > 32) ? 32 : ct;
                    a.LDY = a.CT + 4;
                    const int r = pair_rows_fit(sizes[z], nbuf * a.LDH + a.LDY);
                    if (r >= (pass == 0 ? want : need)) { *rows = r; return z; }
                }
        *rows = 0;
        return -1;
    };
}

inline size_t plm_pw(int H, int C, int layers) { return (layers == 2 ? (size_t)H * H : 0) + (size_t)H * C; }
inline int plm_bq_blocks(size_t PW) { return pair_bq_blocks(PW, PLM_BQ_BLOCKS, PLM_BQ_BLOCKS_MIN); }
struct PlmSpace { size_t partial, wpartial, coef, inv_nn, ties, total, PD, PW; };
inline PlmSpace plm_space(int n, int H, int C, int layers)
{
    const size_t rows = (size_t)(n > 0 ? n : 0), WT = (size_t)layers * H + C;
    PlmSpace s;
    s.PD = 2 * WT + 3 * (size_t)H;
    s.PW = plm_pw(H, C, layers);
    s.partial = 0;
    s.wpartial = pair_up256(sizeof(double) * (size_t)(PLM_F_BLOCKS > PLM_BQ_BLOCKS ? PLM_F_BLOCKS : PLM_BQ_BLOCKS) * s.PD);
    s.coef = s.wpartial + pair_up256(sizeof(float) * (size_t)plm_bq_blocks(s.PW) * s.PW);
    s.inv_nn = s.coef + pair_up256(sizeof(float) * 2 * WT);
    s.ties = s.inv_nn + pair_up256(sizeof(float) * rows);
    s.total = s.ties + pair_up256(sizeof(float) * rows * C);
    return s;
}

inline PlmArgs plm_args(int n, int n0, int K, int H, int C, int layers, const float* q, const float* s, const int* idx, const float* cen, const float* nbr,
                        const float* wp, const float* hw, float radius, int bn_mode, const float* gamma, const float* beta, const float* mean, const float* invstd,
                        int act, int red, const int* padding_num)
{
    PlmArgs a;
    a.n = n; a.n0 = n0; a.K = K; a.H = H; a.HP = pair_up16(H); a.LDH = a.HP; a.nct = a.HP / 16; a.C = C; a.L = layers; a.WT = layers * H + C;
    a.act = act; a.bn = bn_mode; a.red = red; a.R = 16; a.tq = 1; a.tpt = 1; a.CT = 16; a.LDY = 20; a.nbuf = layers;
    a.q = q; a.s = s; a.idx = idx; a.cen = cen; a.nbr = nbr; a.wp = wp; a.hw = hw; a.gamma = gamma; a.beta = beta; a.mean = mean; a.invstd = invstd;
    a.inv_radius = 1.0f / radius; a.padding_num = padding_num;
    return a;
}

}  // namespace

#define PLM_LAUNCH(kernel, z, ...) PAIR_LAUNCH(kernel, z, PLM_LDS0, PLM_LDS1, PLM_LDS2, __VA_ARGS__)

CBL_EXPORT size_t cbl_pointwise_mlp_layers_workspace_bytes(int n, int n0, int K, int H, int C_out, int layers)
{
    if (plm_check(n, n0, K, H, C_out, layers, 1.f, 0, 0, 0) != CBL_OK) return 0;
    return plm_space(n, H, C_out, layers).total + 256;
}

CBL_EXPORT int cbl_pointwise_mlp_layers_forward(int n, int n0, int K, int H, int C_out, const float* query_points, const float* support_points,
                                                const int* neighbors_indices, const float* center_term, const float* neighbor_term, const float* w_pos,
                                                float radius, int layers, const float* hidden_w, int bn_mode, const float* gamma, const float* beta, float eps,
                                                float momentum, float* moving_mean, float* moving_var, int activation, int reduction, const int* padding_num,
                                                float* save_mean, float* save_invstd, float* out, void* workspace, size_t workspace_bytes, void* stream)
{
    const int rc = plm_check(n, n0, K, H, C_out, layers, radius, bn_mode, activation, reduction);
    if (rc) return rc;
    if (n == 0) return CBL_OK;
    if (!query_points || !support_points || !neighbors_indices || !hidden_w || !out || (reduction == PAIR_MEAN && !padding_num)) return CBL_ERR_BAD_ARG;
    if (bn_mode != PLM_BN_NONE && (!save_mean || !save_invstd || !(eps > 0.f))) return CBL_ERR_BAD_ARG;
    if (bn_mode == PLM_BN_MOVING && (!moving_mean || !moving_var)) return CBL_ERR_BAD_ARG;
    if (bn_mode == PLM_BN_BATCH && (!workspace || !cbl_host_aligned16(workspace))) return CBL_ERR_BAD_ARG;
    if (bn_mode == PLM_BN_BATCH && workspace_bytes < cbl_pointwise_mlp_layers_workspace_bytes(n, n0, K, H, C_out, layers)) return CBL_ERR_WORKSPACE;
    hipStream_t st = cbl_stream(stream);
    PlmArgs a = plm_args(n, n0, K, H, C_out, layers, query_points, support_points, neighbors_indices, center_term, neighbor_term, w_pos, hidden_w, radius,
                         bn_mode, gamma, beta, save_mean, save_invstd, activation, reduction, padding_num);
    const int z = pair_plan_query(a, plm_plan(a, layers));
    if (z < 0) return CBL_ERR_UNSUPPORTED;
    const PlmSpace sp = plm_space(n, H, C_out, layers);
    const unsigned g = cbl_grid_for(n, a.tq, PLM_F_BLOCKS);
    if (bn_mode == PLM_BN_BATCH) {
        double* partial = reinterpret_cast<double*>(workspace);
        const double N = (double)n * (double)K;
        for (int l = 0; l <= layers; l++) {                           // the statistics of layer l, with those of the layers below it final
            const int off = l * H, width = l < layers ? H : C_out;
            PLM_LAUNCH(plm_forward_kernel, z, dim3(g), st, a, l, partial, sp.PD, (float*)nullptr);
            hipLaunchKernelGGL(plm_fin_stats_kernel, dim3(cbl_div_up(width, 256)), dim3(256), 0, st, off, width, a.WT, (int)g, sp.PD, (const double*)partial, N, eps,
                               momentum, moving_mean, moving_var, save_mean, save_invstd);
        }
    } else if (bn_mode == PLM_BN_MOVING) {
        hipLaunchKernelGGL(plm_moving_kernel, dim3(cbl_div_up(a.WT, 256)), dim3(256), 0, st, a.WT, (const float*)moving_mean, (const float*)moving_var, eps,
                           save_mean, save_invstd);
    }
    PLM_LAUNCH(plm_forward_kernel, z, dim3(g), st, a, layers + 1, (double*)nullptr, sp.PD, out);
    return cbl_status();
}

CBL_EXPORT int cbl_pointwise_mlp_layers_backward_csr(int n, int n0, int K, int H, int C_out, const float* query_points, const float* support_points,
                                                     const int* neighbors_indices, const float* center_term, const float* neighbor_term, const float* w_pos,
                                                     float radius, int layers, const float* hidden_w, int bn_mode, const float* gamma, const float* beta,
                                                     const float* save_mean, const float* save_invstd, int activation, int reduction, const int* padding_num,
                                                     const float* out, const float* grad_out, const int* order_dst, const int* inv_start, const int* inv_src,
                                                     float* grad_center, float* grad_neighbor, float* grad_w_pos, float* grad_hidden_w, float* grad_gamma,
                                                     float* grad_beta, void* workspace, size_t workspace_bytes, void* stream)
{
    const int rc = plm_check(n, n0, K, H, C_out, layers, radius, bn_mode, activation, reduction);
    if (rc) return rc;
    if (!grad_center && !grad_neighbor && !grad_w_pos && !grad_hidden_w && !grad_gamma && !grad_beta) return CBL_OK;
    if (n > 0 && (!query_points || !support_points || !neighbors_indices || !hidden_w || !grad_out || (reduction == PAIR_MEAN && !padding_num) ||
                  (reduction == PAIR_MAX && !out))) return CBL_ERR_BAD_ARG;
    if (bn_mode != PLM_BN_NONE && (!save_mean || !save_invstd)) return CBL_ERR_BAD_ARG;
    const bool table = grad_neighbor && n0 > 0;
    if (table && (!inv_start || !inv_src || !support_points)) return CBL_ERR_BAD_ARG;
    if (grad_w_pos && !w_pos) return CBL_ERR_BAD_ARG;
    if (!workspace || !cbl_host_aligned16(workspace)) return CBL_ERR_BAD_ARG;
    if (workspace_bytes < cbl_pointwise_mlp_layers_workspace_bytes(n, n0, K, H, C_out, layers)) return CBL_ERR_WORKSPACE;
    hipStream_t st = cbl_stream(stream);
    const PlmSpace sp = plm_space(n, H, C_out, layers);
    const size_t WT = (size_t)layers * H + C_out;
    if (n == 0) {                                                    // no pair: every sum is empty
        if (grad_neighbor && n0 > 0) (void)hipMemsetAsync(grad_neighbor, 0, sizeof(float) * (size_t)n0 * H, st);
        if (grad_w_pos) (void)hipMemsetAsync(grad_w_pos, 0, sizeof(float) * 3 * (size_t)H, st);
        if (grad_hidden_w) (void)hipMemsetAsync(grad_hidden_w, 0, sizeof(float) * sp.PW, st);
        if (grad_gamma) (void)hipMemsetAsync(grad_gamma, 0, sizeof(float) * WT, st);
        if (grad_beta) (void)hipMemsetAsync(grad_beta, 0, sizeof(float) * WT, st);
        return cbl_status();
    }
    char* base = reinterpret_cast<char*>(workspace);
    double* partial = reinterpret_cast<double*>(base + sp.partial);
    float* wpartial = grad_hidden_w ? reinterpret_cast<float*>(base + sp.wpartial) : nullptr;
    float* coef = reinterpret_cast<float*>(base + sp.coef);
    PlmArgs a = plm_args(n, n0, K, H, C_out, layers, query_points, support_points, neighbors_indices, center_term, neighbor_term, w_pos, hidden_w, radius,
                         bn_mode, gamma, beta, save_mean, save_invstd, activation, reduction, padding_num);
    PlmBwd b;
    b.go = grad_out; b.out = out; b.coef = coef;
    b.inv_nn = reinterpret_cast<float*>(base + sp.inv_nn); b.ties = reinterpret_cast<float*>(base + sp.ties);
    const int zq = pair_plan_query(a, plm_plan(a, layers + 1));
    if (zq < 0) return CBL_ERR_UNSUPPORTED;
    const unsigned gq = cbl_grid_for(n, a.tq, plm_bq_blocks(sp.PW));
    const double N = (double)n * (double)K;
    const int wpos = grad_w_pos ? 1 : 0;
    if (bn_mode == PLM_BN_BATCH) {
        for (int lo = layers; lo >= 0; lo--) {                        // the sums of layer lo, with those of the layers above it final
            const int off = lo * H, width = lo < layers ? H : C_out;
            PLM_LAUNCH(plm_bwd_query_kernel, zq, dim3(gq), st, a, b, lo, lo == layers ? 1 : 0, partial, sp.PD, wpartial, sp.PW, (float*)nullptr, 0);
            hipLaunchKernelGGL(plm_fin_bn_kernel, dim3(cbl_div_up(width, 256)), dim3(256), 0, st, off, width, a.WT, (int)gq, sp.PD, (const double*)partial, N,
                               grad_gamma, grad_beta, coef);
        }
        PLM_LAUNCH(plm_bwd_query_kernel, zq, dim3(gq), st, a, b, -1, 0, partial, sp.PD, wpartial, sp.PW, grad_center, wpos);
    } else {
        PLM_LAUNCH(plm_bwd_query_kernel, zq, dim3(gq), st, a, b, -1, 1, partial, sp.PD, wpartial, sp.PW, grad_center, wpos);
        if (bn_mode == PLM_BN_MOVING)
            hipLaunchKernelGGL(plm_fin_bn_kernel, dim3(cbl_div_up(a.WT, 256)), dim3(256), 0, st, 0, a.WT, a.WT, (int)gq, sp.PD, (const double*)partial, N,
                               grad_gamma, grad_beta, coef);
    }
    if (grad_hidden_w || grad_w_pos)
        hipLaunchKernelGGL(plm_fin_w_kernel, dim3(cbl_grid_for((long long)(sp.PW + 3 * (size_t)H), 256, 1024)), dim3(256), 0, st, H, a.WT, (int)gq, sp.PW, sp.PD,
                           (const float*)wpartial, (const double*)partial, grad_hidden_w, grad_w_pos);
    if (table) {
        const int zt = pair_plan_target(a, plm_plan(a, layers + 1));
        if (zt < 0) return CBL_ERR_UNSUPPORTED;
        a.tq = 0;
        PLM_LAUNCH(plm_bwd_target_kernel, zt, dim3(cbl_grid_for(n0, a.tpt, PLM_BT_BLOCKS)), st, a, b, cbl_fastdiv_make((unsigned)K), order_dst, inv_start,
                   inv_src, grad_neighbor);
    }
    return cbl_status();
}

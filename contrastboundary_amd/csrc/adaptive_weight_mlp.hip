// a14: AdaptiveWeight with fc_num 2 and 3 — a per-pair MLP of width M between the folded first layer and the weights.
// tensorflow/models/local_aggregation_operators.py:356, 419-430: fc_0 (the fold of adaptive_weight_general.hip, then the activation), fc_1 .. fc_{fc_num-2}
// ((M, M) with bias and activation, no batch norm), fc_{fc_num} ((M, M) with bias, no activation).  For the pair (i, k), j = idx[i, k], L = fc_num - 1:
//     y0[m] = ((s_j - q_i) / radius) . W_p[:,m] + Cen[idx[i,0]][m] + Nbr[j][m] + b0[m]          h = act(y0)
//     h = act(h @ W_l + b_l)   l = 1 .. L-1                                                      y = h @ W_L + b_L
// and from y on everything is the general operator: weight_softmax None / masked / 'unmask', the reshape-multiply by f_j in groups of S = C / M, sum / mean /
// max with the -65535 shadow value and the padding_num quirk (see the header comment of adaptive_weight_general.hip).  Shadow pairs go through the MLP like
// any other (zero rows, their point at the origin).  act: 1 relu, 2 leaky_relu (alpha 0.2), anything else the identity (basic_operators.py:285-289).
//
// MI355X mapping.  The product h @ W crosses the lanes, so the pairs of a few queries are a small dense matrix in LDS: a workgroup (four waves) takes a tile of
// whole queries per trip, R = their pair rows padded to a multiple of 16, the M columns zero-padded to MP = a multiple of 16 inside the kernel.  The row
// convention, the y0 fold, the weight-gradient tiles, the target-side chunk walk and the host-side tile planning are pair_tile.h's, shared with
// pointwise_mlp_layers.hip; the layer product keeps pair_tile.h's lane layout in a loop of its own (awm_layer).
//   rows    : the y0 rows are made on the VALU (one thread per (row, column)) into LDS
//   layers  : a wave owns its 16-row tile across all MP / 16 column tiles (accumulators in registers), so the forward pass runs the layers in place.
//             The weights are the B operand, read from global memory (at most 2 x 81 KB, shared by every workgroup: L2 / L1 resident)
//   weights : a thread per (query, group) walks the K logits of its column in LDS: running max / sum, then y -> w in place
//   reduce  : a thread per (query, float4 of channels) walks the K pairs: w from LDS, f_j from memory
//   forward   F : rows, layers, weights, reduce -> out
//   backward  BQ: by query, the forward again with h of every layer kept (layers + 1 buffers); ties of 'max'; a thread per (query, group) forms dw, D = sum_k w dw
//                 and dy = w (dw - D) in place of w; then per layer from the last: grad_hidden_w += h^T dz on MFMA (the pairs are the contraction) into the
//                 workgroup's own fp32 partial, column sums for the biases, dz <- (dz @ W^T) * act'(h) on MFMA in place of h.  At the first layer:
//                 grad_center = sum_k dz0, partial sums of grad_w_pos and grad_bias0.  lse, D, 1 / nn and the ties go to the workspace.
//                 A finalize kernel adds the workgroups' partials in a fixed order in fp64.
//             BT: by target, over the transposed table: chunks of R pairs of a trip's targets recompute the forward (and, when grad_neighbor is asked for, the
//                 backward walk to dz0) reading lse / D / 1 / nn / ties; a thread per (target, float4) sums da w, a thread per (target, column) sums dz0.
// Under a softmax sum_k dy = 0 exactly: the LAST layer's bias gradient is written as zeros.  That shortcut does not hold for the first layer any more
// (the activation sits between): grad_center and grad_bias0 are computed.
// No float atomics; every output is stored by one thread in a fixed order.  LDS: one of three static sizes (24 / 56 / 96 KB of rows + 7 KB of row data), the
// smallest that holds a useful tile — gfx950 has 160 KB per compute unit; rows are MP + 4 floats apart where the tile still fits (the 16 rows of an A operand
// then fall into different banks), MP where not.
#include "pair_tile.h"

namespace {

enum { AWM_SM_NONE = 0, AWM_SM_MASKED = 1, AWM_SM_UNMASK = 2 };
constexpr int AWM_MMIN = 16, AWM_MMAX = 144, AWM_KMAX = 128, AWM_KWIDE = 48, AWM_MNARROW = 64, AWM_CMAX = 1152;
// grid caps (four workgroups of the smallest LDS size per compute unit: a trip is a chain of short phases behind barriers, other workgroups fill its waits);
// BQ's also bounds the partials: at most PAIR_BQ_PARTIAL floats of them, never fewer than AWM_BQ_BLOCKS_MIN workgroups
constexpr int AWM_F_BLOCKS = 1024, AWM_BQ_BLOCKS = 1024, AWM_BQ_BLOCKS_MIN = 256, AWM_BT_BLOCKS = 1024;
constexpr int AWM_LDS0 = 6144, AWM_LDS1 = 14336, AWM_LDS2 = 24576;                                 // floats of row buffers
constexpr float AWM_SHADOW_MAX = -65535.f;                                                         // :475

struct AwmArgs {
    int n, n0, K, C, M, S, MP, LD, nct, layers, act, softmax, red;
    int R, tq, tpt;                             // rows of a tile (a multiple of 16), queries of a trip (F, BQ), targets of a trip (BT)
    const float* q; const float* s; const int* idx; const float* f;
    const float* cen; const float* nbr; const float* wp; const float* b0; const float* hw; const float* hb;
    float inv_radius;
    const int* padding_num;
};
struct AwmBwd {
    const float* go; const float* out;
    float* lse; float* D; float* inv_nn; float* ties;
};
struct AwmLds { float* buf; float* dp; int* rowI; int* rowJ; int* rowC; float* cnt; };

#define AWM_LDS_DECL(L)                                                                                                              \
    __shared__ float awm_buf[LDSF]; __shared__ float awm_dp[PAIR_RMAX * 3]; __shared__ int awm_ri[PAIR_RMAX]; __shared__ int awm_rj[PAIR_RMAX]; \
    __shared__ int awm_rc[PAIR_RMAX]; __shared__ float awm_cnt[PAIR_RMAX];                                                            \
    AwmLds L; L.buf = awm_buf; L.dp = awm_dp; L.rowI = awm_ri; L.rowJ = awm_rj; L.rowC = awm_rc; L.cnt = awm_cnt

__device__ __forceinline__ bool awm_in(int softmax, bool real) { return softmax != AWM_SM_MASKED || real; }
__device__ __forceinline__ void awm_ld4(const float* p, float (&v)[4])
{
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void awm_st4(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }

// One layer on MFMA, a wave per 16-row tile with every column tile's accumulator in registers: pair_mfma's loop and lane layout, written out.  As two calls
// of pair_mfma the compiler re-evaluated the lanes' column test inside the k loop (one vector compare per MFMA) instead of keeping the nine masks, and the
// passes at M = 72 and 144 measured 1.5 % to 4 % slower on the MI355X (profiles/pair_tile_refactor.md); this text compiles to the loop it always had.
//   BACK false: out = act(in @ W + bias)          (in == out allowed: the tile's rows are read before they are written)
//   BACK true : out = (in @ W^T) * act'(out)      (out holds the layer's input h on entry, the gradient at its pre-activation on exit)
// Columns past M read zero weights and are written as zero.
template <bool BACK>
__device__ __forceinline__ void awm_layer(const AwmArgs& a, const float* in, float* out, const float* __restrict__ W, const float* __restrict__ bias, int act)
{
    const int wave = threadIdx.x / CBL_WAVE, lane = threadIdx.x % CBL_WAVE, li = lane % 16, lk = lane / 16;
    for (int t = wave; t < a.R / 16; t += PAIR_WAVES) {
        pair_f32x4 acc[PAIR_NCT];
#pragma unroll
        for (int c = 0; c < PAIR_NCT; c++) acc[c] = pair_f32x4{0.f, 0.f, 0.f, 0.f};
        const float* arow = in + (16 * t + li) * a.LD;
#pragma unroll 4
        for (int k0 = 0; k0 < a.MP; k0 += 4) {                             // (MP / 4 is a multiple of 4: no remainder loop; four steps' loads in flight)
            const int kk = k0 + lk;
            const float av = arow[kk];
#pragma unroll
            for (int c = 0; c < PAIR_NCT; c++) {
                if (c >= a.nct) continue;
                const int col = 16 * c + li;
                const float bv = (kk < a.M && col < a.M) ? (BACK ? W[(size_t)col * a.M + kk] : W[(size_t)kk * a.M + col]) : 0.f;
                acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[c], 0, 0, 0);
            }
        }
#pragma unroll
        for (int c = 0; c < PAIR_NCT; c++) {
            if (c >= a.nct) continue;
            const int col = 16 * c + li;
#pragma unroll
            for (int v = 0; v < 4; v++) {
                float* o = out + (16 * t + 4 * lk + v) * a.LD + col;
                float val = 0.f;
                if (col < a.M) val = BACK ? acc[c][v] * pair_dact(act, *o) : pair_act(act, acc[c][v] + bias[col]);
                *o = val;
            }
        }
    }
}

// rows -> y: fc_0 and its activation into buffer 0 (act(y0 + b0)), then the layers; keep: layer l writes buffer l (the backward pass reads every h),
// otherwise in place.  Ends behind a barrier.
__device__ __forceinline__ float* awm_chain(const AwmArgs& a, const AwmLds& L, bool keep)
{
    pair_fold_rows(a, L, a.M, a.MP, a.wp, a.cen, a.nbr, L.buf, a.LD, [&](int m, float y0) { return pair_act(a.act, y0 + a.b0[m]); });
    __syncthreads();
    float* in = L.buf;
    for (int l = 1; l <= a.layers; l++) {
        float* out = keep ? L.buf + (size_t)l * a.R * a.LD : L.buf;
        awm_layer<false>(a, in, out, a.hw + (size_t)(l - 1) * a.M * a.M, a.hb + (size_t)(l - 1) * a.M, l < a.layers ? a.act : 0);
        __syncthreads();
        in = out;
    }
    return in;
}

// dz of the last layer (in buffer `layers`) back to dz0 in buffer 0; between the steps `between(l, h, dz)` sees layer l's input h and the gradient dz at
// its output (BQ: the weight and bias sums).  Starts and ends behind a barrier.
template <class F>
__device__ __forceinline__ void awm_walk_back(const AwmArgs& a, const AwmLds& L, F between)
{
    for (int l = a.layers; l >= 1; l--) {
        float* dz = L.buf + (size_t)l * a.R * a.LD;
        float* h = L.buf + (size_t)(l - 1) * a.R * a.LD;
        between(l, h, dz);
        awm_layer<true>(a, dz, h, a.hw + (size_t)(l - 1) * a.M * a.M, nullptr, a.act);
        __syncthreads();
    }
}

// a query's K logits of one column -> its weights in place (running max and sum: no overflow whatever the logits); lse_out: kept for BT
__device__ __forceinline__ void awm_weights_query(const AwmArgs& a, const AwmLds& L, int i0, float* Y, float* __restrict__ lse_out)
{
    if (a.softmax == AWM_SM_NONE) return;
    for (int it = threadIdx.x; it < a.tq * a.M; it += PAIR_BLOCK) {
        const int qi = it / a.M, m = it - qi * a.M, i = i0 + qi;
        if (i >= a.n) continue;
        float* col = Y + (size_t)qi * a.K * a.LD + m;
        const int* rj = L.rowJ + qi * a.K;
        float mx = -INFINITY, sm = 0.f;
        for (int k = 0; k < a.K; k++) {
            if (!awm_in(a.softmax, pair_real(rj[k], a.n0))) continue;
            const float y = col[k * a.LD];
            if (y > mx) { sm = sm * expf(mx - y) + 1.f; mx = y; }
            else sm += expf(y - mx);
        }
        const float lse = mx + logf(sm);                                 // (empty domain: -inf, never read)
        if (lse_out) lse_out[(size_t)i * a.M + m] = lse;
        for (int k = 0; k < a.K; k++) col[k * a.LD] = awm_in(a.softmax, pair_real(rj[k], a.n0)) ? expf(col[k * a.LD] - lse) : 0.f;
    }
}

// the gradient at a[i,k,c] of a REAL pair: grad_out / nn, or grad_out / ties where the pair's product wf attains the maximum
__device__ __forceinline__ float awm_da(const AwmArgs& a, const AwmBwd& b, size_t at, float sc, float wf)
{
    const float g = b.go[at];
    if (a.red != PAIR_MAX) return g * sc;
    const float tc = b.ties[at];
    return (wf == b.out[at] && tc > 0.f) ? g / tc : 0.f;
}
// dw of the pair in row r at group m: the sum over the group's S channels, in channel order
__device__ __forceinline__ float awm_dw(const AwmArgs& a, const AwmBwd& b, int i, int id, int m, float sc, float w)
{
    const float* __restrict__ fj = a.f + (size_t)id * a.C + (size_t)m * a.S;
    const size_t at = (size_t)i * a.C + (size_t)m * a.S;
    float dw = 0.f;
    for (int e = 0; e < a.S; e++) dw += awm_da(a, b, at + e, sc, w * fj[e]) * fj[e];
    return dw;
}

// ---------------------------------------------------------------- F
template <int LDSF>
__global__ __launch_bounds__(PAIR_BLOCK) void awm_forward_kernel(AwmArgs a, float* __restrict__ out)
{
    AWM_LDS_DECL(L);
    const int pad = (a.red == PAIR_MEAN) ? *a.padding_num : 0;
    const int ntrips = (a.n + a.tq - 1) / a.tq, U = a.C / 4;
    for (int trip = blockIdx.x; trip < ntrips; trip += gridDim.x) {
        const int i0 = trip * a.tq;
        pair_rows_query(a, L, i0, pad);
        __syncthreads();
        float* Y = awm_chain(a, L, false);
        awm_weights_query(a, L, i0, Y, nullptr);
        __syncthreads();
        for (int it = threadIdx.x; it < a.tq * U; it += PAIR_BLOCK) {
            const int qi = it / U, c0 = 4 * (it - qi * U), i = i0 + qi;
            if (i >= a.n) continue;
            int me[4];
            float acc[4];
#pragma unroll
            for (int e = 0; e < 4; e++) { me[e] = (c0 + e) / a.S; acc[e] = a.red == PAIR_MAX ? -INFINITY : 0.f; }
#pragma unroll 4
            for (int k = 0; k < a.K; k++) {
                const int r = qi * a.K + k, id = L.rowJ[r];
                const bool real = pair_real(id, a.n0);
                float f4[4] = {0.f, 0.f, 0.f, 0.f};
                if (real) awm_ld4(a.f + (size_t)id * a.C + c0, f4);
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const float av = real ? Y[r * a.LD + me[e]] * f4[e] : (a.red == PAIR_MAX ? AWM_SHADOW_MAX : 0.f);      // :458, :475-477
                    if (a.red == PAIR_MAX) acc[e] = av > acc[e] ? av : acc[e]; else acc[e] += av;
                }
            }
            if (a.red == PAIR_MEAN) {
                const float nn = L.cnt[qi] + 1e-5f;                      // :466-470
#pragma unroll
                for (int e = 0; e < 4; e++) acc[e] = acc[e] / nn;
            }
            awm_st4(out + (size_t)i * a.C + c0, acc);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- BQ
// partial: this workgroup's fp32 sums, [layers M M | 3 M grad_w_pos | M grad_bias0 | layers M grad_hidden_b] (PS floats per workgroup)
template <int LDSF>
__global__ __launch_bounds__(PAIR_BLOCK) void awm_bwd_query_kernel(AwmArgs a, AwmBwd b, float* __restrict__ grad_center, float* __restrict__ partial, size_t PS)
{
    AWM_LDS_DECL(L);
    const int pad = (a.red == PAIR_MEAN) ? *a.padding_num : 0;
    const int ntrips = (a.n + a.tq - 1) / a.tq, U = a.C / 4;
    const bool sm = a.softmax != AWM_SM_NONE;
    float* mine = partial ? partial + (size_t)blockIdx.x * PS : nullptr;
    double gb[3] = {0.0, 0.0, 0.0}, T[3] = {0.0, 0.0, 0.0};             // thread m < M: the column sums of dz at layer 0, 1, 2 and of dp^T dz0
    for (int trip = blockIdx.x; trip < ntrips; trip += gridDim.x) {
        const int i0 = trip * a.tq;
        const bool first = trip == (int)blockIdx.x;
        pair_rows_query(a, L, i0, pad);
        __syncthreads();
        float* Y = awm_chain(a, L, true);
        awm_weights_query(a, L, i0, Y, b.lse);
        for (int qi = threadIdx.x; qi < a.tq; qi += PAIR_BLOCK)
            if (i0 + qi < a.n) b.inv_nn[i0 + qi] = a.red == PAIR_MEAN ? 1.0f / (L.cnt[qi] + 1e-5f) : 1.0f;
        __syncthreads();
        if (a.red == PAIR_MAX) {                                          // how many pairs attain each maximum
            for (int it = threadIdx.x; it < a.tq * U; it += PAIR_BLOCK) {
                const int qi = it / U, c0 = 4 * (it - qi * U), i = i0 + qi;
                if (i >= a.n) continue;
                int me[4];
                float m4[4], tc[4] = {0.f, 0.f, 0.f, 0.f};
                awm_ld4(b.out + (size_t)i * a.C + c0, m4);
#pragma unroll
                for (int e = 0; e < 4; e++) me[e] = (c0 + e) / a.S;
                for (int k = 0; k < a.K; k++) {
                    const int r = qi * a.K + k, id = L.rowJ[r];
                    const bool real = pair_real(id, a.n0);
                    float f4[4] = {0.f, 0.f, 0.f, 0.f};
                    if (real) awm_ld4(a.f + (size_t)id * a.C + c0, f4);
#pragma unroll
                    for (int e = 0; e < 4; e++) tc[e] += ((real ? Y[r * a.LD + me[e]] * f4[e] : AWM_SHADOW_MAX) == m4[e]) ? 1.f : 0.f;
                }
                awm_st4(b.ties + (size_t)i * a.C + c0, tc);
            }
            __syncthreads();
        }
        // w -> dy in place: dw per pair, D = sum_k w dw, dy = w (dw - D) formed per pair (a query with one real neighbour has dy = 0 exactly)
        for (int it = threadIdx.x; it < a.tq * a.MP; it += PAIR_BLOCK) {
            const int qi = it / a.MP, m = it - qi * a.MP, i = i0 + qi;
            float* col = Y + (size_t)qi * a.K * a.LD + m;
            if (i >= a.n || m >= a.M) {
                for (int k = 0; k < a.K; k++) col[k * a.LD] = 0.f;
                continue;
            }
            const int* rj = L.rowJ + qi * a.K;
            const float sc = a.red == PAIR_MEAN ? 1.0f / (L.cnt[qi] + 1e-5f) : 1.0f;
            float D = 0.f;
            if (sm) {
                for (int k = 0; k < a.K; k++)
                    if (pair_real(rj[k], a.n0)) D += col[k * a.LD] * awm_dw(a, b, i, rj[k], m, sc, col[k * a.LD]);
                b.D[(size_t)i * a.M + m] = D;
            }
            for (int k = 0; k < a.K; k++) {
                const bool real = pair_real(rj[k], a.n0);
                const float w = col[k * a.LD];
                const float dw = real ? awm_dw(a, b, i, rj[k], m, sc, w) : 0.f;
                col[k * a.LD] = sm ? (awm_in(a.softmax, real) ? w * (dw - D) : 0.f) : dw;
            }
        }
        for (int it = a.tq * a.K * a.MP + threadIdx.x; it < a.R * a.MP; it += PAIR_BLOCK)       // the rows behind the last query: no gradient
            Y[(it / a.MP) * a.LD + it % a.MP] = 0.f;
        __syncthreads();
        awm_walk_back(a, L, [&](int l, const float* h, const float* dz) {
            if (!mine) return;
            // grad_hidden_w[l-1][p][c] += sum_r h[r][p] dz[r][c]
            pair_wgrad(a.R, a.nct, a.M, [&](int r, int p) { return h[r * a.LD + p]; }, dz, a.LD, a.nct, a.M, mine + (size_t)(l - 1) * a.M * a.M, a.M, 0, first);
            if ((int)threadIdx.x < a.M) {
                float s = 0.f;
                for (int r = 0; r < a.R; r++) s += dz[r * a.LD + threadIdx.x];
                gb[l] += (double)s;
            }
            __syncthreads();
        });
        // dz0 in buffer 0
        if (grad_center) {
            for (int it = threadIdx.x; it < a.tq * a.M; it += PAIR_BLOCK) {
                const int qi = it / a.M, m = it - qi * a.M, i = i0 + qi;
                if (i >= a.n) continue;
                float s = 0.f;
                for (int k = 0; k < a.K; k++) s += L.buf[(qi * a.K + k) * a.LD + m];
                grad_center[(size_t)i * a.M + m] = s;
            }
        }
        if (mine && (int)threadIdx.x < a.M) {
            float s = 0.f, t0 = 0.f, t1 = 0.f, t2 = 0.f;
            for (int r = 0; r < a.R; r++) {
                const float dz = L.buf[r * a.LD + threadIdx.x];
                s += dz; t0 += L.dp[3 * r] * dz; t1 += L.dp[3 * r + 1] * dz; t2 += L.dp[3 * r + 2] * dz;
            }
            gb[0] += (double)s; T[0] += (double)t0; T[1] += (double)t1; T[2] += (double)t2;
        }
        __syncthreads();
    }
    if (mine && (int)threadIdx.x < a.M) {
        float* pv = mine + (size_t)a.layers * a.M * a.M;
        const int m = threadIdx.x;
        for (int d = 0; d < 3; d++) pv[d * a.M + m] = (float)T[d];
        pv[3 * a.M + m] = (float)gb[0];
        for (int l = 1; l <= a.layers; l++) pv[(3 + l) * a.M + m] = (float)gb[l];
    }
}

// the workgroups' partials, added in the order of the workgroups in fp64; under a softmax the last layer's bias gradient is exactly 0
__global__ __launch_bounds__(256) void awm_finalize_kernel(int M, int layers, int nblocks, size_t PS, const float* __restrict__ partial, float* __restrict__ grad_hw,
                                                           float* __restrict__ grad_w_pos, float* __restrict__ grad_b0, float* __restrict__ grad_hb,
                                                           int zero_last_bias)
{
    const size_t nw = (size_t)layers * M * M;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < PS; e += (size_t)gridDim.x * 256) {
        double s = 0.0;
        for (int bk = 0; bk < nblocks; bk++) s += (double)partial[(size_t)bk * PS + e];
        const float v = (float)s;
        if (e < nw) { if (grad_hw) grad_hw[e] = v; continue; }
        const size_t o = e - nw;
        if (o < (size_t)3 * M) { if (grad_w_pos) grad_w_pos[o] = v; }
        else if (o < (size_t)4 * M) { if (grad_b0) grad_b0[o - 3 * M] = v; }
        else if (grad_hb) grad_hb[o - 4 * M] = (zero_last_bias && o - 4 * M >= (size_t)(layers - 1) * M) ? 0.f : v;
    }
}

// ---------------------------------------------------------------- BT
template <int LDSF>
__global__ __launch_bounds__(PAIR_BLOCK) void awm_bwd_target_kernel(AwmArgs a, AwmBwd b, CblFastDiv dvK, const int* __restrict__ order,
                                                                   const int* __restrict__ inv_start, const int* __restrict__ inv_src,
                                                                   float* __restrict__ grad_neighbor, float* __restrict__ grad_value)
{
    AWM_LDS_DECL(L);
    const bool sm = a.softmax != AWM_SM_NONE, walk = grad_neighbor != nullptr;
    const int ntrips = (a.n0 + a.tpt - 1) / a.tpt, U = a.C / 4;
    for (int trip = blockIdx.x; trip < ntrips; trip += gridDim.x) {
        const int t_lo = trip * a.tpt, t_hi = min(t_lo + a.tpt, a.n0);
        const int e_lo = inv_start[t_lo], e_hi = inv_start[t_hi];
        int ce = e_lo;
        do {                                                             // chunks of R pairs; at least one, so that a target without pairs is stored too
            const bool last = ce + a.R >= e_hi;
            pair_rows_target(a, L, dvK, inv_src, ce, e_hi);
            __syncthreads();
            float* Y = awm_chain(a, L, walk);
            if (sm) {
                for (int it = threadIdx.x; it < a.R * a.M; it += PAIR_BLOCK) {
                    const int r = it / a.M, m = it - r * a.M, i = L.rowI[r];
                    if (i >= 0) Y[r * a.LD + m] = expf(Y[r * a.LD + m] - b.lse[(size_t)i * a.M + m]);
                }
                __syncthreads();
            }
            if (grad_value) {                                            // grad_features_value[j, c] = sum over j's pairs of da w
                for (int it = threadIdx.x; it < a.tpt * U; it += PAIR_BLOCK) {
                    const int tl = it / U, c0 = 4 * (it - tl * U), tr = t_lo + tl;
                    if (tr >= t_hi) continue;
                    const int s0 = inv_start[tr], s1 = inv_start[tr + 1];
                    bool begins;
                    if (!pair_target_in_chunk(s0, s1, ce, a.R, last, &begins)) continue;
                    const int j = order ? order[tr] : tr;
                    int me[4];
                    float acc[4] = {0.f, 0.f, 0.f, 0.f}, f4[4];
                    awm_ld4(a.f + (size_t)j * a.C + c0, f4);
#pragma unroll
                    for (int e = 0; e < 4; e++) me[e] = (c0 + e) / a.S;
                    for (int e = max(s0, ce); e < min(s1, ce + a.R); e++) {
                        const int r = e - ce, i = L.rowI[r];
                        const float sc = b.inv_nn[i];
#pragma unroll
                        for (int c = 0; c < 4; c++) {
                            const float w = Y[r * a.LD + me[c]];
                            acc[c] += awm_da(a, b, (size_t)i * a.C + c0 + c, sc, w * f4[c]) * w;
                        }
                    }
                    float* dst = grad_value + (size_t)j * a.C + c0;
                    if (!begins) {
                        float old[4];
                        awm_ld4(dst, old);
#pragma unroll
                        for (int c = 0; c < 4; c++) acc[c] = old[c] + acc[c];
                    }
                    awm_st4(dst, acc);
                }
            }
            if (walk) {
                __syncthreads();
                for (int it = threadIdx.x; it < a.R * a.MP; it += PAIR_BLOCK) {      // w -> dy in place
                    const int r = it / a.MP, m = it - r * a.MP, i = L.rowI[r];
                    float dy = 0.f;
                    if (i >= 0 && m < a.M) {
                        const float w = Y[r * a.LD + m];
                        const float dw = awm_dw(a, b, i, L.rowJ[r], m, b.inv_nn[i], w);
                        dy = sm ? w * (dw - b.D[(size_t)i * a.M + m]) : dw;
                    }
                    Y[r * a.LD + m] = dy;
                }
                __syncthreads();
                awm_walk_back(a, L, [](int, const float*, const float*) {});
                pair_target_sum(a, a.M, L.buf, a.LD, t_lo, t_hi, ce, last, order, inv_start, grad_neighbor);      // grad_neighbor[j, m] = sum over j's pairs of dz0
            }
            __syncthreads();
            ce += a.R;
        } while (ce < e_hi);
    }
}

// ---------------------------------------------------------------- host side
int awm_check(int n, int n0, int K, int C, int M, int layers, float radius, int softmax, int reduction)
{
    if (n < 0 || n0 < 0 || K <= 0 || C <= 0 || M <= 0 || layers < 0 || !(radius > 0.f)) return CBL_ERR_BAD_ARG;
    if (softmax < 0 || softmax > AWM_SM_UNMASK || reduction < 0 || reduction > PAIR_MAX) return CBL_ERR_BAD_ARG;
    if (layers < 1 || layers > 2 || K > AWM_KMAX || C % 4 != 0 || C > AWM_CMAX || C % M != 0) return CBL_ERR_UNSUPPORTED;
    if (M < AWM_MMIN || M > AWM_MMAX || (K > AWM_KWIDE && M > AWM_MNARROW)) return CBL_ERR_UNSUPPORTED;
    const int S = C / M;
    if (!(S == 1 || S == 2 || S == 4 || S % 4 == 0)) return CBL_ERR_UNSUPPORTED;
    return CBL_OK;
}

// the LDS size (0, 1, 2) and the rows of a tile for `nbuf` row buffers: the smallest size that holds `want` rows, else the smallest that holds `need`
inline int awm_plan(int LD, int nbuf, int need, int want, int* rows)
{
    const int sizes[3] = {AWM_LDS0, AWM_LDS1, AWM_LDS2};
    for (int pass = 0; pass < 2; pass++)
        for (int z = 0; z < 3; z++) {
            const int r = pair_rows_fit(sizes[z], nbuf * LD);
            if (r >= (pass == 0 ? want : need)) { *rows = r; return z; }
        }
    *rows = 0;
    return -1;
}
// the plan of pair_plan_query / pair_plan_target for `nbuf` row buffers: rows of MP + 4 floats (the 16 rows an MFMA operand reads then fall into 16
// different groups of 4 banks) where a tile still fits, MP where not.  The callable writes the pitch it chose into a.LD: use it within the expression
// that makes it, on the args object that is launched
inline auto awm_plan_rows(AwmArgs& a, int nbuf)
{
    return [&a, nbuf](int need, int want, int* rows) {
        a.LD = a.MP + 4;
        int z = awm_plan(a.LD, nbuf, need, want, rows);
        if (z < 0) { a.LD = a.MP; z = awm_plan(a.LD, nbuf, need, want, rows); }
        return z;
    };
}

inline int awm_bq_blocks(size_t PS) { return pair_bq_blocks(PS, AWM_BQ_BLOCKS, AWM_BQ_BLOCKS_MIN); }
struct AwmSpace { size_t partial, lse, D, inv_nn, ties, total, PS; };
inline AwmSpace awm_space(int n, int C, int M, int layers)
{
    const size_t rows = (size_t)(n > 0 ? n : 0);
    AwmSpace s;
    s.PS = (size_t)layers * M * M + (size_t)(4 + layers) * M;
    s.partial = 0;
    s.lse = pair_up256(sizeof(float) * (size_t)awm_bq_blocks(s.PS) * s.PS);
    s.D = s.lse + pair_up256(sizeof(float) * rows * M);
    s.inv_nn = s.D + pair_up256(sizeof(float) * rows * M);
    s.ties = s.inv_nn + pair_up256(sizeof(float) * rows);
    s.total = s.ties + pair_up256(sizeof(float) * rows * C);
    return s;
}

inline AwmArgs awm_args(int n, int n0, int K, int C, int M, int layers, int act, const float* q, const float* s, const int* idx, const float* f, const float* cen,
                        const float* nbr, const float* wp, const float* b0, const float* hw, const float* hb, float radius, int softmax, int red,
                        const int* padding_num)
{
    AwmArgs a;
    a.n = n; a.n0 = n0; a.K = K; a.C = C; a.M = M; a.S = C / M; a.MP = pair_up16(M); a.LD = a.MP; a.nct = a.MP / 16; a.layers = layers; a.act = act;
    a.softmax = softmax; a.red = red; a.R = 16; a.tq = 1; a.tpt = 1;
    a.q = q; a.s = s; a.idx = idx; a.f = f; a.cen = cen; a.nbr = nbr; a.wp = wp; a.b0 = b0; a.hw = hw; a.hb = hb; a.inv_radius = 1.0f / radius;
    a.padding_num = padding_num;
    return a;
}

}  // namespace

#define AWM_LAUNCH(kernel, z, ...) PAIR_LAUNCH(kernel, z, AWM_LDS0, AWM_LDS1, AWM_LDS2, __VA_ARGS__)

CBL_EXPORT size_t cbl_adaptive_weight_mlp_workspace_bytes(int n, int n0, int K, int C, int M, int layers)
{
    if (awm_check(n, n0, K, C, M, layers, 1.f, 0, 0) != CBL_OK) return 0;
    return awm_space(n, C, M, layers).total + 256;
}

CBL_EXPORT int cbl_adaptive_weight_mlp_forward(int n, int n0, int K, int C, int M, const float* query_points, const float* support_points,
                                               const int* neighbors_indices, const float* features, const float* center_term, const float* neighbor_term,
                                               const float* w_pos, const float* bias, int layers, const float* hidden_w, const float* hidden_b, int activation,
                                               float radius, int softmax, int reduction, const int* padding_num, float* out, void* workspace,
                                               size_t workspace_bytes, void* stream)
{
    (void)workspace; (void)workspace_bytes;                           // (the forward pass keeps its rows in LDS)
    const int rc = awm_check(n, n0, K, C, M, layers, radius, softmax, reduction);
    if (rc) return rc;
    if (n == 0) return CBL_OK;
    if (!query_points || !support_points || !neighbors_indices || !features || !bias || !hidden_w || !hidden_b || !out ||
        (reduction == PAIR_MEAN && !padding_num)) return CBL_ERR_BAD_ARG;
    if (!cbl_host_aligned16(features) || !cbl_host_aligned16(out)) return CBL_ERR_UNSUPPORTED;
    hipStream_t st = cbl_stream(stream);
    AwmArgs a = awm_args(n, n0, K, C, M, layers, activation, query_points, support_points, neighbors_indices, features, center_term, neighbor_term, w_pos, bias,
                         hidden_w, hidden_b, radius, softmax, reduction, padding_num);
    const int z = pair_plan_query(a, awm_plan_rows(a, 1));
    if (z < 0) return CBL_ERR_UNSUPPORTED;
    AWM_LAUNCH(awm_forward_kernel, z, dim3(cbl_grid_for(n, a.tq, AWM_F_BLOCKS)), st, a, out);
    return cbl_status();
}

CBL_EXPORT int cbl_adaptive_weight_mlp_backward_csr(int n, int n0, int K, int C, int M, const float* query_points, const float* support_points,
                                                    const int* neighbors_indices, const float* features, const float* center_term, const float* neighbor_term,
                                                    const float* w_pos, const float* bias, int layers, const float* hidden_w, const float* hidden_b,
                                                    int activation, float radius, int softmax, int reduction, const int* padding_num, const float* out,
                                                    const float* grad_out, const int* order_dst, const int* inv_start, const int* inv_src,
                                                    float* grad_features_value, float* grad_center, float* grad_neighbor, float* grad_w_pos, float* grad_bias,
                                                    float* grad_hidden_w, float* grad_hidden_b, void* workspace, size_t workspace_bytes, void* stream)
{
    const int rc = awm_check(n, n0, K, C, M, layers, radius, softmax, reduction);
    if (rc) return rc;
    if (!grad_features_value && !grad_center && !grad_neighbor && !grad_w_pos && !grad_bias && !grad_hidden_w && !grad_hidden_b) return CBL_OK;
    if (n > 0 && (!query_points || !support_points || !neighbors_indices || !features || !bias || !hidden_w || !hidden_b || !grad_out ||
                  (reduction == PAIR_MEAN && !padding_num) || (reduction == PAIR_MAX && !out))) return CBL_ERR_BAD_ARG;
    const bool table = (grad_features_value || grad_neighbor) && n0 > 0;
    if (table && (!inv_start || !inv_src || !support_points || !features)) return CBL_ERR_BAD_ARG;
    if (!workspace || !cbl_host_aligned16(workspace)) return CBL_ERR_BAD_ARG;
    if (workspace_bytes < cbl_adaptive_weight_mlp_workspace_bytes(n, n0, K, C, M, layers)) return CBL_ERR_WORKSPACE;
    if (!cbl_host_aligned16(features) || !cbl_host_aligned16(out) || !cbl_host_aligned16(grad_out) || !cbl_host_aligned16(grad_features_value))
        return CBL_ERR_UNSUPPORTED;
    hipStream_t st = cbl_stream(stream);
    if (n == 0) {                                                    // no pair: every sum is empty
        if (grad_features_value && n0 > 0) (void)hipMemsetAsync(grad_features_value, 0, sizeof(float) * (size_t)n0 * C, st);
        if (grad_neighbor && n0 > 0) (void)hipMemsetAsync(grad_neighbor, 0, sizeof(float) * (size_t)n0 * M, st);
        if (grad_w_pos) (void)hipMemsetAsync(grad_w_pos, 0, sizeof(float) * 3 * (size_t)M, st);
        if (grad_bias) (void)hipMemsetAsync(grad_bias, 0, sizeof(float) * (size_t)M, st);
        if (grad_hidden_w) (void)hipMemsetAsync(grad_hidden_w, 0, sizeof(float) * (size_t)layers * M * M, st);
        if (grad_hidden_b) (void)hipMemsetAsync(grad_hidden_b, 0, sizeof(float) * (size_t)layers * M, st);
        return cbl_status();
    }
    const AwmSpace sp = awm_space(n, C, M, layers);
    char* base = reinterpret_cast<char*>(workspace);
    float* partial = reinterpret_cast<float*>(base + sp.partial);
    AwmArgs a = awm_args(n, n0, K, C, M, layers, activation, query_points, support_points, neighbors_indices, features, center_term, neighbor_term, w_pos, bias,
                         hidden_w, hidden_b, radius, softmax, reduction, padding_num);
    AwmBwd b;
    b.go = grad_out; b.out = out;
    b.lse = reinterpret_cast<float*>(base + sp.lse); b.D = reinterpret_cast<float*>(base + sp.D);
    b.inv_nn = reinterpret_cast<float*>(base + sp.inv_nn); b.ties = reinterpret_cast<float*>(base + sp.ties);
    const bool sums = grad_w_pos || grad_bias || grad_hidden_w || grad_hidden_b;
    const int zq = pair_plan_query(a, awm_plan_rows(a, layers + 1));
    if (zq < 0) return CBL_ERR_UNSUPPORTED;
    const unsigned gq = cbl_grid_for(n, a.tq, awm_bq_blocks(sp.PS));
    AWM_LAUNCH(awm_bwd_query_kernel, zq, dim3(gq), st, a, b, grad_center, sums ? partial : (float*)nullptr, sp.PS);
    if (sums)
        hipLaunchKernelGGL(awm_finalize_kernel, dim3(cbl_grid_for((long long)sp.PS, 256, 256)), dim3(256), 0, st, M, layers, (int)gq, sp.PS, (const float*)partial,
                           grad_hidden_w, grad_w_pos, grad_bias, grad_hidden_b, softmax != AWM_SM_NONE ? 1 : 0);
    if (table) {
        const int zt = pair_plan_target(a, awm_plan_rows(a, grad_neighbor ? layers + 1 : 1));
        if (zt < 0) return CBL_ERR_UNSUPPORTED;
        AWM_LAUNCH(awm_bwd_target_kernel, zt, dim3(cbl_grid_for(n0, a.tpt, AWM_BT_BLOCKS)), st, a, b, cbl_fastdiv_make((unsigned)K), order_dst, inv_start,
                   inv_src, grad_neighbor, grad_features_value);
    }
    return cbl_status();
}

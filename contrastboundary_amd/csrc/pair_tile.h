// What the per-pair MLP kernel files (adaptive_weight_mlp.hip, pointwise_mlp_layers.hip) share: a workgroup of four waves takes a tile of whole queries
// (or, on the target side, a chunk of the transposed neighbour table) per trip; the tile's pairs are the rows of a small dense matrix in LDS.
//   rows    : row r of a tile is one pair.  rowI = its query, -1 on a row past the trip's pairs (such a row enters no sum and is stored as zeros);
//             rowJ = its neighbour id, a shadow pair has rowJ >= n0 and its point at the origin; rowC = idx[i, 0], the query's centre row;
//             dp = (s_j - q_i) / radius.
//   y_0     : the folded first layer of one (row, column) is ONE expression with ONE association (pair_fold_y0): 'max' compares products that every pass
//             recomputes, so they have to come out to the same bits.
//   layers  : per 16-row tile a chain of v_mfma_f32_16x16x4_f32 (an exact fp32 fmaf chain).  A[i][k] in lane i + 16 k, B[k][j] in lane 16 k + j,
//             D[4 (lane / 16) + v][lane % 16] in element v.
//   targets : a target whose pairs span several chunks is continued by the same thread of the same workgroup (stored at its first chunk, added to
//             afterwards): no float atomics, one fixed order.
// The library is built with -ffp-contract=off: an expression keeps its rounding wherever it is inlined, as long as its parentheses are kept.
// The grid caps and the LDS sizes differ between the two files and stay there.
#pragma once
#include "cbl_common.h"

namespace {

typedef float pair_f32x4 __attribute__((vector_size(16)));

enum { PAIR_SUM = 0, PAIR_MEAN = 1, PAIR_MAX = 2 };                   // the `red` of both files' entries (PAIR_SUM: the value neither of the others)
// threads and waves of a workgroup, the most rows of a tile, the most 16-column tiles a wave keeps in registers (widths up to 144), the most targets of a
// target-side trip, the most floats of the query-side backward's weight partials
constexpr int PAIR_BLOCK = 256, PAIR_WAVES = 4, PAIR_RMAX = 256, PAIR_NCT = 9, PAIR_TPT_MAX = 16, PAIR_BQ_PARTIAL = 1 << 24;

// Both files' argument structs name the geometry of a launch alike — n, n0, K, R (rows of a tile, a multiple of 16), tq (queries of a trip, query side), tpt
// (targets of a trip, target side), red, q, s, idx, inv_radius, padding_num — and their LDS structs the row part — dp[3 PAIR_RMAX], rowI / rowJ / rowC /
// cnt[PAIR_RMAX].  The functions below are templates over those structs (class A, class ROWS) and use these members only: the structs keep their own field
// order, so a kernel's argument segment is laid out as its file wrote it.  (Two shared base structs were tried first: the geometry then came first in
// the argument segment, the scalar loads and the register allocation of every kernel moved, and single shapes measured 0.5 % to 0.8 % slower on the
// MI355X.  With the templates the forward kernels and PointWiseMLP's query kernels compile to the instructions they had before the header existed.)

__device__ __forceinline__ bool pair_real(int id, int n0) { return id >= 0 && id < n0; }
__device__ __forceinline__ float pair_act(int act, float z) { return act == 1 ? (z > 0.f ? z : 0.f) : act == 2 ? (z > 0.f ? z : 0.2f * z) : z; }
// the activation's slope, from its input z or from its OUTPUT h alike (h > 0 exactly where z > 0): adaptive_weight_mlp.hip passes h, pointwise_mlp_layers.hip z
__device__ __forceinline__ float pair_dact(int act, float z) { return act == 1 ? (z > 0.f ? 1.f : 0.f) : act == 2 ? (z > 0.f ? 1.f : 0.2f) : 1.f; }

// the rows of a query trip: row r = (query i0 + r / K, neighbour r % K); cnt[qi] = the count behind 'mean' (indices below pad = max(idx))
template <class A, class ROWS>
__device__ __forceinline__ void pair_rows_query(const A& a, const ROWS& L, int i0, int pad)
{
    for (int r = threadIdx.x; r < a.R; r += PAIR_BLOCK) {
        const int qi = r / a.K, k = r - qi * a.K, i = i0 + qi;
        const bool valid = qi < a.tq && i < a.n;
        int id = -1;
        float d0 = 0.f, d1 = 0.f, d2 = 0.f;
        if (valid) {
            id = a.idx[(size_t)i * a.K + k];
            float sx = 0.f, sy = 0.f, sz = 0.f;
            if (pair_real(id, a.n0)) { sx = a.s[3 * (size_t)id]; sy = a.s[3 * (size_t)id + 1]; sz = a.s[3 * (size_t)id + 2]; }
            d0 = (sx - a.q[3 * (size_t)i]) * a.inv_radius; d1 = (sy - a.q[3 * (size_t)i + 1]) * a.inv_radius; d2 = (sz - a.q[3 * (size_t)i + 2]) * a.inv_radius;
        }
        L.rowI[r] = valid ? i : -1; L.rowJ[r] = id; L.rowC[r] = valid ? a.idx[(size_t)i * a.K] : -1;
        L.dp[3 * r] = d0; L.dp[3 * r + 1] = d1; L.dp[3 * r + 2] = d2;
    }
    for (int qi = threadIdx.x; qi < a.tq; qi += PAIR_BLOCK) {
        const int i = i0 + qi;
        int cnt = 0;
        if (i < a.n && a.red == PAIR_MEAN)
            for (int k = 0; k < a.K; k++) cnt += (a.idx[(size_t)i * a.K + k] < pad) ? 1 : 0;
        L.cnt[qi] = (float)cnt;
    }
}

// the rows of a target chunk: row r = entry ce + r of the transposed table, below e_hi.  The table holds real targets only (j < n0): s[j] is read
// without the pair_real test
template <class A, class ROWS>
__device__ __forceinline__ void pair_rows_target(const A& a, const ROWS& L, CblFastDiv dvK, const int* __restrict__ inv_src, int ce, int e_hi)
{
    for (int r = threadIdx.x; r < a.R; r += PAIR_BLOCK) {
        const int e = ce + r;
        int i = -1, j = -1;
        float d0 = 0.f, d1 = 0.f, d2 = 0.f;
        if (e < e_hi) {
            const int p = inv_src[e];
            i = (int)cbl_fastdiv((unsigned)p, dvK);
            j = a.idx[p];
            d0 = (a.s[3 * (size_t)j] - a.q[3 * (size_t)i]) * a.inv_radius; d1 = (a.s[3 * (size_t)j + 1] - a.q[3 * (size_t)i + 1]) * a.inv_radius;
            d2 = (a.s[3 * (size_t)j + 2] - a.q[3 * (size_t)i + 2]) * a.inv_radius;
        }
        L.rowI[r] = i; L.rowJ[r] = j; L.rowC[r] = i >= 0 ? a.idx[(size_t)i * a.K] : -1;
        L.dp[3 * r] = d0; L.dp[3 * r + 1] = d1; L.dp[3 * r + 2] = d2;
    }
}

// y_0 of (row r, column m < W) without a bias: dp . w_pos[:, m] + cen[rowC][m] + nbr[rowJ][m]; a null term, a shadow centre or neighbour add 0
template <class A, class ROWS>
__device__ __forceinline__ float pair_fold_y0(const A& a, const ROWS& L, int r, int m, int W, const float* __restrict__ wp,
                                              const float* __restrict__ cen, const float* __restrict__ nbr)
{
    const int id = L.rowJ[r], c0 = L.rowC[r];
    const float w0 = wp ? wp[m] : 0.f, w1 = wp ? wp[W + m] : 0.f, w2 = wp ? wp[2 * W + m] : 0.f;
    const float ce = (cen && pair_real(c0, a.n0)) ? cen[(size_t)c0 * W + m] : 0.f;
    const float nb = (nbr && pair_real(id, a.n0)) ? nbr[(size_t)id * W + m] : 0.f;
    return (((L.dp[3 * r] * w0 + L.dp[3 * r + 1] * w1) + L.dp[3 * r + 2] * w2) + ce) + nb;
}
// X[r][m] = finish(m, y_0) for every row of the tile and m < WP (X's rows ld apart), zero on the padding rows and columns: one thread per (row, column)
template <class A, class ROWS, class F>
__device__ __forceinline__ void pair_fold_rows(const A& a, const ROWS& L, int W, int WP, const float* __restrict__ wp, const float* __restrict__ cen,
                                               const float* __restrict__ nbr, float* __restrict__ X, int ld, F finish)
{
#pragma unroll 4
    for (int it = threadIdx.x; it < a.R * WP; it += PAIR_BLOCK) {
        const int r = it / WP, m = it - r * WP, i = L.rowI[r];
        float v = 0.f;
        if (i >= 0 && m < W) v = finish(m, pair_fold_y0(a, L, r, m, W, wp, cen, nbr));
        X[r * ld + m] = v;
    }
}

// A product on MFMA, a wave per 16-row tile with every column tile's accumulator in registers: acc(row, col) = fi(row, col) + sum_k fa(row, k) fb(k, col),
// k < KP (a multiple of 4), handed to fe(row, col, value).  A wave reads all of its tile's operands before fe runs, and the tiles of different waves are
// different rows: fe may overwrite what fa read.  (adaptive_weight_mlp.hip's awm_layer is this loop written out: see there.)
template <int NCT, class FA, class FB, class FI, class FE>
__device__ __forceinline__ void pair_mfma(int R, int KP, int nct, FA fa, FB fb, FI fi, FE fe)
{
    const int wave = threadIdx.x / CBL_WAVE, lane = threadIdx.x % CBL_WAVE, li = lane % 16, lk = lane / 16;
    for (int t = wave; t < R / 16; t += PAIR_WAVES) {
        pair_f32x4 acc[NCT];
#pragma unroll
        for (int c = 0; c < NCT; c++) {
            acc[c] = pair_f32x4{0.f, 0.f, 0.f, 0.f};
            if (c >= nct) continue;
#pragma unroll
            for (int v = 0; v < 4; v++) acc[c][v] = fi(16 * t + 4 * lk + v, 16 * c + li);
        }
#pragma unroll 4
        for (int k0 = 0; k0 < KP; k0 += 4) {                                   // (four steps' loads in flight)
            const int kk = k0 + lk;
            const float av = fa(16 * t + li, kk);
#pragma unroll
            for (int c = 0; c < NCT; c++) {
                if (c >= nct) continue;
                acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, fb(kk, 16 * c + li), acc[c], 0, 0, 0);
            }
        }
#pragma unroll
        for (int c = 0; c < NCT; c++) {
            if (c >= nct) continue;
#pragma unroll
            for (int v = 0; v < 4; v++) fe(16 * t + 4 * lk + v, 16 * c + li, acc[c][v]);
        }
    }
}

// A weight gradient, the pairs being the contraction: dst[p][col0 + c] (+)= sum_{r < R} h(r, p) D[r][c] for p < P (ntp = P / 16 rounded up), c < cw (ntc
// tiles); tile (tp, tc) of wave (tp ntc + tc) % 4, continued from the workgroup's own fp32 partial unless `first`
template <class FH>
__device__ __forceinline__ void pair_wgrad(int R, int ntp, int P, FH h, const float* D, int ldd, int ntc, int cw, float* __restrict__ dst, int ldw, int col0,
                                           bool first)
{
    const int wave = threadIdx.x / CBL_WAVE, lane = threadIdx.x % CBL_WAVE, li = lane % 16, lk = lane / 16;
    for (int tile = wave; tile < ntp * ntc; tile += PAIR_WAVES) {
        const int tp = tile / ntc, tc = tile - tp * ntc, col = 16 * tc + li;
        pair_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (!first) {
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const int p = 16 * tp + 4 * lk + v;
                if (p < P && col < cw) acc[v] = dst[(size_t)p * ldw + col0 + col];
            }
        }
        for (int r0 = 0; r0 < R; r0 += 4)
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(h(r0 + lk, 16 * tp + li), D[(r0 + lk) * ldd + col], acc, 0, 0, 0);
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const int p = 16 * tp + 4 * lk + v;
            if (p < P && col < cw) dst[(size_t)p * ldw + col0 + col] = acc[v];
        }
    }
}

// Does the chunk [ce, ce + R) concern the target whose table entries are [s0, s1)?  begins: the target is STORED here — its first entry lies in the chunk, or
// it has none left to come and this is the trip's last chunk (a target without pairs is stored too); otherwise the chunk's share is added to what is stored
__device__ __forceinline__ bool pair_target_in_chunk(int s0, int s1, int ce, int R, bool last, bool* begins)
{
    *begins = s0 >= ce && (s0 < ce + R || last);
    return *begins || (s0 < ce && s1 > ce);
}
// dst[j, m] (+)= the sum over target j's rows of the chunk of DY[row][m], m < W: a thread per (target of the trip, column)
template <class A>
__device__ __forceinline__ void pair_target_sum(const A& a, int W, const float* DY, int ld, int t_lo, int t_hi, int ce, bool last,
                                                const int* __restrict__ order, const int* __restrict__ inv_start, float* __restrict__ dst_rows)
{
    for (int it = threadIdx.x; it < a.tpt * W; it += PAIR_BLOCK) {
        const int tl = it / W, m = it - tl * W, tr = t_lo + tl;
        if (tr >= t_hi) continue;
        const int s0 = inv_start[tr], s1 = inv_start[tr + 1];
        bool begins;
        if (!pair_target_in_chunk(s0, s1, ce, a.R, last, &begins)) continue;
        const int j = order ? order[tr] : tr;
        float s = 0.f;
        for (int e = max(s0, ce); e < min(s1, ce + a.R); e++) s += DY[(e - ce) * ld + m];
        float* dst = dst_rows + (size_t)j * W + m;
        *dst = begins ? s : *dst + s;
    }
}

// ---------------------------------------------------------------- host side
inline int pair_up16(int v) { return (v + 15) / 16 * 16; }
inline size_t pair_up256(size_t b) { return (b + 255) & ~(size_t)255; }
// the rows of a tile that `floats` of LDS hold at `per_row` floats a row
inline int pair_rows_fit(int floats, int per_row)
{
    const int r = floats / per_row / 16 * 16;
    return r > PAIR_RMAX ? PAIR_RMAX : r;
}
// workgroups of the query-side backward: its weight partials (PS floats each) stay within PAIR_BQ_PARTIAL floats, between the file's two caps
inline int pair_bq_blocks(size_t PS, int blocks_max, int blocks_min)
{
    const size_t fit = (size_t)PAIR_BQ_PARTIAL / PS;
    return fit > (size_t)blocks_max ? blocks_max : fit < (size_t)blocks_min ? blocks_min : (int)fit;
}
// plan(need, want, &rows) -> the LDS size (0, 1, 2; < 0: none fits) and the rows it holds; the file's plan also writes the row pitches it chose into
// the SAME args object whose tq / R / tpt are set here.  A query pass: as many whole queries as the rows hold
template <class A, class PLAN>
inline int pair_plan_query(A& a, PLAN plan)
{
    int rows;
    const int z = plan(pair_up16(a.K), pair_up16(a.K) > 64 ? pair_up16(a.K) : 64, &rows);
    if (z < 0) return z;
    a.tq = rows / a.K;
    if (a.n > 0 && a.tq > a.n) a.tq = a.n;
    a.R = pair_up16(a.tq * a.K);
    return z;
}
// a target pass (n0 > 0: the caller launches it only where there is a table): a trip's targets are about one tile of pairs at the table's mean segment
// length (the chunk loop takes whatever a trip really has)
template <class A, class PLAN>
inline int pair_plan_target(A& a, PLAN plan)
{
    int rows;
    const int z = plan(16, 128, &rows);
    if (z < 0) return z;
    a.R = rows;
    const long long mean = ((long long)a.n * a.K + a.n0 - 1) / a.n0;
    const long long tpt = rows / (mean > 0 ? mean : 1);
    a.tpt = (int)(tpt < 1 ? 1 : tpt > PAIR_TPT_MAX ? PAIR_TPT_MAX : tpt);
    return z;
}

}  // namespace

// kernel<L0 | L1 | L2> for the LDS size z = 0 | 1 | 2
#define PAIR_LAUNCH(kernel, z, L0, L1, L2, grid, st, ...)                                                                            \
    do {                                                                                                                             \
        if ((z) == 0) hipLaunchKernelGGL(kernel<L0>, grid, dim3(PAIR_BLOCK), 0, st, __VA_ARGS__);                                    \
        else if ((z) == 1) hipLaunchKernelGGL(kernel<L1>, grid, dim3(PAIR_BLOCK), 0, st, __VA_ARGS__);                               \
        else hipLaunchKernelGGL(kernel<L2>, grid, dim3(PAIR_BLOCK), 0, st, __VA_ARGS__);                                             \
    } while (0)

// a14: AdaptiveWeight, the whole option space of fc_num 1 — feature-driven weights, shared channels, softmax over the neighbours, 'max'.
// Replaces the TF1 op chain of AdaptiveWeight  tensorflow/models/local_aggregation_operators.py:316-500 (local_input_feature 'dp' | 'df' | 'dp_df' | 'fj' |
// 'dp_fj' | 'fi_df' | 'dp_fi_df' :386-401, batch_conv1d_1x1 `fc_1` with bias :426-430, weight_softmax :432-453, the reshape-multiply :455-459 and the
// reduction :461-480).  The shipped configuration ('dp', shared_channels 1, no softmax, sum / mean) keeps its own kernels (local_aggregation.hip).
// With C channels in M = C / S groups of S = shared_channels, one FC layer is linear in the concatenated blocks, so for the pair (i, k), j = idx[i, k]:
//     y[i,k,m] = ((s_j - q_i) / radius) . W_p[:,m]  +  Cen[idx[i,0]][m]  +  Nbr[j][m]  +  bias[m]      Cen = features @ (W_fi - W_df), Nbr = features @ (W_df + W_fj)
// (two per-point (n0, M) products made by the caller; shadow rows are zero, the shadow point is the origin), then
//     w = y | softmax_k over the real pairs ('dense' / 'sparse' / 'mask') | softmax_k over all K pairs ('unmask');   a[i,k,c] = w[i,k,c/S] * f_j[c]
//     out[i,c] = sum_k a | sum_k a / nn[i] | max_k (a, -65535 on a shadow pair)
// Every pass RECOMPUTES y from the gathered Nbr row, the query's Cen row and a 3 x M product; nothing of shape (n, K, .) exists in memory.
//
// MI355X mapping.  A lane owns whole weight groups: for S in {1, 2, 4} one float4 of channels = 4 / S groups (G = 4, 2, 1), for S % 4 == 0 one group that it
// walks in S / 4 float4 steps.  The gradient at a weight, dw[i,k,m] = sum over the S channels of the group, is then a sum inside the lane for every S — the
// other cut (a lane = 4 channels of any group) needs a reduction over S / 4 lanes per PAIR in the target-side pass, and S / 4 is no power of two (6, 18).
// The C / max(S, 4) lanes of a row sit next to each other (for S <= 4 a neighbour's row is one contiguous burst); a row wider than 256 lanes is walked in
// column blocks (blockIdx.y).  A group wider than the accumulators a lane can hold is walked in chunks of float4 steps, the logits recomputed per chunk.
//   forward   F : per query the running max / sum of the logits (one walk), then weight, multiply and reduce (second walk) -> out
//   backward  BQ: per query the log-normaliser (n, M), D[i,m] = sum_k w dw (n, M), 1 / nn (n), the tie counts of 'max' (n, C) -> workspace;
//                 grad_center (n, M) = sum_k dy, per-workgroup fp64 partials of grad_w_pos = sum dp^T dy and grad_bias = sum dy, finalised in a fixed order
//             BT: per target j of the transposed table, every pair of its segment recomputes y, w, da, dw, dy = w (dw - D):
//                 grad_neighbor[j] = sum dy, grad_features_value[j] = sum da w, each stored once
// A softmax is invariant under a shift of its K logits, so under any softmax sum_k dy = 0 EXACTLY: grad_center and grad_bias are written as zeros there
// (computing D - D * sum_k w would leave rounding noise where the true value is 0).
// No float atomics: partial sums are combined in a fixed order (fp64), every output is stored once.
#include "cbl_common.h"

namespace {

enum { AWG_SM_NONE = 0, AWG_SM_MASKED = 1, AWG_SM_UNMASK = 2 };
enum { AWG_SUM = 0, AWG_MEAN = 1, AWG_MAX = 2 };
constexpr int AWG_KMAX = 128, AWG_CMAX = 1152, AWG_BLOCK = 256, AWG_MAX_BLOCKS = 512;
constexpr int AWG_FIN_M = 8, AWG_FIN_SLICES = 32;                  // the finalize workgroup: 8 groups x 32 slices of the partials
constexpr float AWG_SHADOW_MAX = -65535.f;                         // :475

struct AwgArgs {
    int n, n0, K, C, M, S;
    int NV, Lr, Lb, tpb;                       // float4 steps of a lane, lanes per row, lanes per row in one column block, rows per workgroup trip
    const float* q; const float* s; const int* idx; const float* f;
    const float* cen; const float* nbr; const float* wp; const float* bias;
    float inv_radius;
    int softmax, red;
    const int* padding_num;
};
struct AwgBwd {                                 // what the backward passes read / write on top
    const float* go; const float* out;
    float* lse; float* D; float* inv_nn; float* ties;
};

template <int G> struct AwgLane { float w[3][G], b[G]; };          // a lane's G weight groups
struct AwgWho { int ts, unit, m0, c0; bool live; };

__device__ __forceinline__ AwgWho awg_who(const AwgArgs& a, int G)
{
    AwgWho w;
    w.ts = threadIdx.x / a.Lb;
    w.unit = blockIdx.y * a.Lb + (threadIdx.x - w.ts * a.Lb);
    w.live = w.ts < a.tpb && w.unit < a.Lr;
    w.m0 = w.unit * G; w.c0 = w.unit * 4 * a.NV;
    return w;
}

__device__ __forceinline__ void awg_ld4(const float* p, float (&v)[4])
{
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void awg_st4(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ bool awg_real(int id, int n0) { return id >= 0 && id < n0; }

template <int G> __device__ __forceinline__ AwgLane<G> awg_lane(const AwgArgs& a, int m0)
{
    AwgLane<G> t;
#pragma unroll
    for (int g = 0; g < G; g++) {
#pragma unroll
        for (int d = 0; d < 3; d++) t.w[d][g] = a.wp ? a.wp[(size_t)d * a.M + m0 + g] : 0.f;
        t.b[g] = a.bias[m0 + g];
    }
    return t;
}
// a (., M) row's G entries of the lane; zero for the shadow row or a block the mode lacks
template <int G> __device__ __forceinline__ void awg_row(const float* tab, int M, int m0, int id, int n0, float (&v)[G])
{
    const bool have = tab && awg_real(id, n0);
#pragma unroll
    for (int g = 0; g < G; g++) v[g] = have ? tab[(size_t)id * M + m0 + g] : 0.f;
}
struct AwgQuery { float qx, qy, qz; };
__device__ __forceinline__ AwgQuery awg_query(const AwgArgs& a, int i)
{
    AwgQuery Q;
    Q.qx = a.q[3 * (size_t)i]; Q.qy = a.q[3 * (size_t)i + 1]; Q.qz = a.q[3 * (size_t)i + 2];
    return Q;
}

// the logits of one pair from its pieces — ONE expression for every pass: 'max' compares a recomputed product with the forward's stored maximum
template <int G>
__device__ __forceinline__ void awg_eval(const AwgLane<G>& t, float inv_radius, float sx, float sy, float sz, const AwgQuery& Q, const float (&cen)[G],
                                         const float (&nb)[G], float (&r)[3], float (&y)[G])
{
    r[0] = (sx - Q.qx) * inv_radius; r[1] = (sy - Q.qy) * inv_radius; r[2] = (sz - Q.qz) * inv_radius;      // :381-382
#pragma unroll
    for (int g = 0; g < G; g++) y[g] = ((((r[0] * t.w[0][g] + r[1] * t.w[1][g]) + r[2] * t.w[2][g]) + cen[g]) + nb[g]) + t.b[g];
}
// the pair (query Q, neighbour id) seen from the query: shadow neighbour = zero rows at the origin (:370-381)
template <int G>
__device__ __forceinline__ bool awg_pair(const AwgArgs& a, const AwgLane<G>& t, int m0, int id, const AwgQuery& Q, const float (&cen)[G], float (&r)[3],
                                         float (&y)[G])
{
    const bool real = awg_real(id, a.n0);
    float sx = 0.f, sy = 0.f, sz = 0.f, nb[G];
    if (real) { sx = a.s[3 * (size_t)id]; sy = a.s[3 * (size_t)id + 1]; sz = a.s[3 * (size_t)id + 2]; }
    awg_row<G>(a.nbr, a.M, m0, id, a.n0, nb);
    awg_eval<G>(t, a.inv_radius, sx, sy, sz, Q, cen, nb, r, y);
    return real;
}
// is the pair inside the softmax's domain (:432-453): every pair without a softmax and under 'unmask', the real pairs under a masked one
__device__ __forceinline__ bool awg_in(int softmax, bool real) { return softmax != AWG_SM_MASKED || real; }
// the weight of a pair: the logit itself, or exp(y - log sum exp) inside the domain and 0 outside (an empty domain has no pair inside)
__device__ __forceinline__ float awg_weight(int softmax, bool in, float y, float lse) { return softmax == AWG_SM_NONE ? y : (in ? expf(y - lse) : 0.f); }

// first walk over a query's K pairs: the log-normaliser of each group (running max and sum: no overflow whatever the logits) and the count behind 'mean'
template <int G>
__device__ __forceinline__ void awg_stats(const AwgArgs& a, const AwgLane<G>& t, int m0, const int* __restrict__ row, const AwgQuery& Q, const float (&cen)[G],
                                          int pad, float (&lse)[G], int& cnt)
{
    float mx[G], sm[G];
#pragma unroll
    for (int g = 0; g < G; g++) { mx[g] = -INFINITY; sm[g] = 0.f; lse[g] = 0.f; }
    cnt = 0;
    if (a.softmax == AWG_SM_NONE) {
        if (a.red == AWG_MEAN)
            for (int k = 0; k < a.K; k++) cnt += (row[k] < pad) ? 1 : 0;
        return;
    }
    for (int k = 0; k < a.K; k++) {
        const int id = row[k];
        cnt += (id < pad) ? 1 : 0;
        float r[3], y[G];
        const bool real = awg_pair<G>(a, t, m0, id, Q, cen, r, y);
        if (!awg_in(a.softmax, real)) continue;
#pragma unroll
        for (int g = 0; g < G; g++) {
            if (y[g] > mx[g]) { sm[g] = sm[g] * expf(mx[g] - y[g]) + 1.f; mx[g] = y[g]; }
            else sm[g] += expf(y[g] - mx[g]);
        }
    }
#pragma unroll
    for (int g = 0; g < G; g++) lse[g] = mx[g] + logf(sm[g]);            // (empty domain: -inf, never read)
}

// ---------------------------------------------------------------- F: weights, multiply, reduce over K
template <int G>
__global__ __launch_bounds__(AWG_BLOCK) void awg_forward_kernel(AwgArgs a, float* __restrict__ out)
{
    constexpr int VB = G == 1 ? 4 : 1, SG = 4 / G;                    // float4 steps per walk; channels of a group inside one float4 (G > 1)
    const AwgWho me = awg_who(a, G);
    if (!me.live) return;
    const AwgLane<G> t = awg_lane<G>(a, me.m0);
    const int pad = (a.red == AWG_MEAN) ? *a.padding_num : 0;
    const int ntrips = (a.n + a.tpb - 1) / a.tpb;
    for (int trip = blockIdx.x; trip < ntrips; trip += gridDim.x) {
        const int i = trip * a.tpb + me.ts;
        if (i >= a.n) continue;
        const AwgQuery Q = awg_query(a, i);
        const int* __restrict__ row = a.idx + (size_t)i * a.K;
        float cen[G], lse[G];
        int cnt;
        awg_row<G>(a.cen, a.M, me.m0, row[0], a.n0, cen);
        awg_stats<G>(a, t, me.m0, row, Q, cen, pad, lse, cnt);
        const float nn = (float)cnt + 1e-5f;                           // :466-470
        for (int v0 = 0; v0 < a.NV; v0 += VB) {
            float acc[VB][4];
#pragma unroll
            for (int u = 0; u < VB; u++)
#pragma unroll
                for (int e = 0; e < 4; e++) acc[u][e] = a.red == AWG_MAX ? -INFINITY : 0.f;
            for (int k = 0; k < a.K; k++) {
                const int id = row[k];
                float r[3], y[G], w[G];
                const bool real = awg_pair<G>(a, t, me.m0, id, Q, cen, r, y);
#pragma unroll
                for (int g = 0; g < G; g++) w[g] = awg_weight(a.softmax, awg_in(a.softmax, real), y[g], lse[g]);
#pragma unroll
                for (int u = 0; u < VB; u++) {
                    if (v0 + u >= a.NV) continue;
                    float f4[4] = {0.f, 0.f, 0.f, 0.f};
                    if (real) awg_ld4(a.f + (size_t)id * a.C + me.c0 + 4 * (v0 + u), f4);
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const float av = real ? w[G == 1 ? 0 : e / SG] * f4[e] : (a.red == AWG_MAX ? AWG_SHADOW_MAX : 0.f);      // :458, :475-477
                        if (a.red == AWG_MAX) acc[u][e] = av > acc[u][e] ? av : acc[u][e]; else acc[u][e] += av;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < VB; u++) {
                if (v0 + u >= a.NV) continue;
                if (a.red == AWG_MEAN) {
#pragma unroll
                    for (int e = 0; e < 4; e++) acc[u][e] = acc[u][e] / nn;
                }
                awg_st4(out + (size_t)i * a.C + me.c0 + 4 * (v0 + u), acc[u]);
            }
        }
    }
}

// the gradient at a[i,k,c] of a REAL pair (i -> j) for the four channels of one float4 step (wf = the pair's products w f_j there): grad_out / nn, or
// grad_out / ties where the pair attains the maximum
__device__ __forceinline__ void awg_da(const AwgArgs& a, const AwgBwd& b, size_t at, float sc, const float (&wf)[4], float (&da)[4])
{
    awg_ld4(b.go + at, da);
    if (a.red == AWG_MAX) {
        float m4[4], tc[4];
        awg_ld4(b.out + at, m4); awg_ld4(b.ties + at, tc);
#pragma unroll
        for (int e = 0; e < 4; e++) da[e] = (wf[e] == m4[e] && tc[e] > 0.f) ? da[e] / tc[e] : 0.f;
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++) da[e] = da[e] * sc;
    }
}

// ---------------------------------------------------------------- BQ: the query side of the backward pass
// First walk(s), per chunk of float4 steps: the tie counts of 'max', and with x[k,c] = 1 on a real pair ('max': on a real pair that attains the maximum) and
// g[c] = grad_out / nn or / ties:  D[m] = sum_{c in m} g[c] sum_k omega x f_j[c]  with omega = w under a softmax ( D = sum_k w dw ) and 1 without
// ( D = sum_k dw = grad_center ) — the factor 1 / ties goes on after the walk, so one walk serves both.
// Last walk: per pair dw (the sum over the lane's S channels, in the order of D's), dy = w (dw - D), grad_w_pos += dp dy.  dy is formed per pair and not as
// a difference of two sums over K: a query with one real neighbour has dy = 0 exactly, as in the graph.
template <int G>
__global__ __launch_bounds__(AWG_BLOCK) void awg_bwd_query_kernel(AwgArgs a, AwgBwd b, float* __restrict__ grad_center, double* __restrict__ partial)
{
    constexpr int VB = G == 1 ? 4 : 1, SG = 4 / G;
    __shared__ double red[4 * G][AWG_BLOCK];
    const AwgWho me = awg_who(a, G);
    double acc[4][G];
#pragma unroll
    for (int r4 = 0; r4 < 4; r4++)
#pragma unroll
        for (int g = 0; g < G; g++) acc[r4][g] = 0.0;
    if (me.live) {
        const AwgLane<G> t = awg_lane<G>(a, me.m0);
        const bool sm = a.softmax != AWG_SM_NONE;
        const int pad = (a.red == AWG_MEAN) ? *a.padding_num : 0;
        const int ntrips = (a.n + a.tpb - 1) / a.tpb;
        for (int trip = blockIdx.x; trip < ntrips; trip += gridDim.x) {
            const int i = trip * a.tpb + me.ts;
            if (i >= a.n) continue;
            const AwgQuery Q = awg_query(a, i);
            const int* __restrict__ row = a.idx + (size_t)i * a.K;
            float cen[G], lse[G], D[G], T[3][G];
            int cnt;
            awg_row<G>(a.cen, a.M, me.m0, row[0], a.n0, cen);
            awg_stats<G>(a, t, me.m0, row, Q, cen, pad, lse, cnt);
            const float scale = a.red == AWG_MEAN ? 1.0f / ((float)cnt + 1e-5f) : 1.0f;
#pragma unroll
            for (int g = 0; g < G; g++) { D[g] = 0.f; T[0][g] = 0.f; T[1][g] = 0.f; T[2][g] = 0.f; }
            for (int v0 = 0; v0 < a.NV; v0 += VB) {
                float E[VB][4], tc[VB][4], m4[VB][4];
#pragma unroll
                for (int u = 0; u < VB; u++) {
#pragma unroll
                    for (int e = 0; e < 4; e++) { tc[u][e] = 0.f; m4[u][e] = 0.f; E[u][e] = 0.f; }
                    if (a.red == AWG_MAX && v0 + u < a.NV) awg_ld4(b.out + (size_t)i * a.C + me.c0 + 4 * (v0 + u), m4[u]);
                }
                for (int k = 0; k < a.K; k++) {
                    const int id = row[k];
                    float r[3], y[G], w[G];
                    const bool real = awg_pair<G>(a, t, me.m0, id, Q, cen, r, y);
#pragma unroll
                    for (int g = 0; g < G; g++) w[g] = awg_weight(a.softmax, awg_in(a.softmax, real), y[g], lse[g]);
#pragma unroll
                    for (int u = 0; u < VB; u++) {
                        if (v0 + u >= a.NV) continue;
                        float f4[4] = {0.f, 0.f, 0.f, 0.f};
                        if (real) awg_ld4(a.f + (size_t)id * a.C + me.c0 + 4 * (v0 + u), f4);
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            const float wf = w[G == 1 ? 0 : e / SG] * f4[e];
                            bool x = real;
                            if (a.red == AWG_MAX) {
                                const bool hit = (real ? wf : AWG_SHADOW_MAX) == m4[u][e];
                                tc[u][e] += hit ? 1.f : 0.f;
                                x = real && hit;
                            }
                            E[u][e] += x ? (sm ? wf : f4[e]) : 0.f;
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < VB; u++) {
                    if (v0 + u >= a.NV) continue;
                    float g4[4];
                    awg_ld4(b.go + (size_t)i * a.C + me.c0 + 4 * (v0 + u), g4);
                    if (a.red == AWG_MAX) awg_st4(b.ties + (size_t)i * a.C + me.c0 + 4 * (v0 + u), tc[u]);
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const float ge = a.red == AWG_MAX ? (tc[u][e] > 0.f ? g4[e] / tc[u][e] : 0.f) : g4[e] * scale;
                        D[G == 1 ? 0 : e / SG] += ge * E[u][e];
                    }
                }
            }
            if (partial) {                                           // grad_w_pos: dy per pair (shadow pairs inside the softmax's domain have dw = 0, dy = -w D)
                for (int k = 0; k < a.K; k++) {
                    const int id = row[k];
                    float r[3], y[G], w[G], dw[G];
                    const bool real = awg_pair<G>(a, t, me.m0, id, Q, cen, r, y);
                    const bool in = awg_in(a.softmax, real);
#pragma unroll
                    for (int g = 0; g < G; g++) { w[g] = awg_weight(a.softmax, in, y[g], lse[g]); dw[g] = 0.f; }
                    if (real) {
                        for (int v = 0; v < a.NV; v++) {
                            float f4[4], wf[4], da[4];
                            awg_ld4(a.f + (size_t)id * a.C + me.c0 + 4 * v, f4);
#pragma unroll
                            for (int e = 0; e < 4; e++) wf[e] = w[G == 1 ? 0 : e / SG] * f4[e];
                            awg_da(a, b, (size_t)i * a.C + me.c0 + 4 * v, scale, wf, da);
#pragma unroll
                            for (int e = 0; e < 4; e++) dw[G == 1 ? 0 : e / SG] += da[e] * f4[e];
                        }
                    }
#pragma unroll
                    for (int g = 0; g < G; g++) {
                        const float dy = sm ? (in ? w[g] * (dw[g] - D[g]) : 0.f) : dw[g];
                        T[0][g] += r[0] * dy; T[1][g] += r[1] * dy; T[2][g] += r[2] * dy;
                    }
                }
            }
#pragma unroll
            for (int g = 0; g < G; g++) {
                if (sm) {
                    b.lse[(size_t)i * a.M + me.m0 + g] = lse[g];
                    b.D[(size_t)i * a.M + me.m0 + g] = D[g];
                }
                if (grad_center) grad_center[(size_t)i * a.M + me.m0 + g] = sm ? 0.f : D[g];      // shift invariance of the softmax: exactly 0
                for (int d = 0; d < 3; d++) acc[d][g] += (double)T[d][g];
                acc[3][g] += sm ? 0.0 : (double)D[g];
            }
            if (me.unit == 0) b.inv_nn[i] = scale;
        }
    }
    if (!partial) return;
    // per-lane sums of the lanes that share a group -> partial[(block * 4 + r) * M + m], in the fixed order of the rows of a workgroup
#pragma unroll
    for (int r4 = 0; r4 < 4; r4++)
#pragma unroll
        for (int g = 0; g < G; g++) red[r4 * G + g][threadIdx.x] = acc[r4][g];
    __syncthreads();
    if (me.live && me.ts == 0) {
        const int ul = threadIdx.x;
        for (int r4 = 0; r4 < 4; r4++)
            for (int g = 0; g < G; g++) {
                double sum = 0.0;
                for (int s = 0; s < a.tpb; s++) sum += red[r4 * G + g][s * a.Lb + ul];
                partial[((size_t)blockIdx.x * 4 + r4) * a.M + me.m0 + g] = sum;
            }
    }
}

// sums of the per-workgroup partials: 8 groups per workgroup, lane (group, slice js) adds every 32nd partial, slices combined through LDS (fp64)
__global__ __launch_bounds__(256) void awg_finalize_kernel(int M, int nblocks, const double* __restrict__ partial, float* __restrict__ grad_w_pos,
                                                           float* __restrict__ grad_bias)
{
    __shared__ double red[AWG_FIN_SLICES][AWG_FIN_M][4];
    const int ms = threadIdx.x % AWG_FIN_M, js = threadIdx.x / AWG_FIN_M, m = blockIdx.x * AWG_FIN_M + ms;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (m < M) {
#pragma unroll 4
        for (int bk = js; bk < nblocks; bk += AWG_FIN_SLICES)
            for (int r = 0; r < 4; r++) s[r] += partial[((size_t)bk * 4 + r) * M + m];
    }
    for (int r = 0; r < 4; r++) red[js][ms][r] = s[r];
    __syncthreads();
    if (js != 0 || m >= M) return;
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < AWG_FIN_SLICES; j++) for (int r = 0; r < 4; r++) t[r] += red[j][ms][r];
    if (grad_w_pos) for (int r = 0; r < 3; r++) grad_w_pos[(size_t)r * M + m] = (float)t[r];
    if (grad_bias) grad_bias[m] = (float)t[3];
}

// ---------------------------------------------------------------- BT: the target side, a gather over the transposed table
template <int G>
__global__ __launch_bounds__(AWG_BLOCK) void awg_bwd_target_kernel(AwgArgs a, AwgBwd b, CblFastDiv dvK, const int* __restrict__ order,
                                                                   const int* __restrict__ inv_start, const int* __restrict__ inv_src,
                                                                   float* __restrict__ grad_neighbor, float* __restrict__ grad_value)
{
    constexpr int VB = G == 1 ? 4 : 1, SG = 4 / G;
    const AwgWho me = awg_who(a, G);
    if (!me.live) return;
    const AwgLane<G> t = awg_lane<G>(a, me.m0);
    const bool sm = a.softmax != AWG_SM_NONE;
    const int ntrips = (a.n0 + a.tpb - 1) / a.tpb;
    for (int trip = blockIdx.x; trip < ntrips; trip += gridDim.x) {
        const int tr = trip * a.tpb + me.ts;
        if (tr >= a.n0) continue;
        const int j = order ? order[tr] : tr;
        const int e0 = inv_start[tr], e1 = inv_start[tr + 1];
        const float sx = a.s[3 * (size_t)j], sy = a.s[3 * (size_t)j + 1], sz = a.s[3 * (size_t)j + 2];
        const float* __restrict__ fj = a.f + (size_t)j * a.C + me.c0;
        float nb[G];
        awg_row<G>(a.nbr, a.M, me.m0, j, a.n0, nb);
        if (grad_neighbor) {                                           // grad_neighbor[j, m] = sum over j's pairs of dy
            float gn[G];
#pragma unroll
            for (int g = 0; g < G; g++) gn[g] = 0.f;
            for (int e = e0; e < e1; e++) {
                const int i = (int)cbl_fastdiv((unsigned)inv_src[e], dvK);
                const AwgQuery Q = awg_query(a, i);
                float cen[G], r[3], y[G], w[G], dw[G];
                awg_row<G>(a.cen, a.M, me.m0, a.idx[(size_t)i * a.K], a.n0, cen);
                awg_eval<G>(t, a.inv_radius, sx, sy, sz, Q, cen, nb, r, y);
#pragma unroll
                for (int g = 0; g < G; g++) { w[g] = awg_weight(a.softmax, true, y[g], sm ? b.lse[(size_t)i * a.M + me.m0 + g] : 0.f); dw[g] = 0.f; }
                const float sc = b.inv_nn[i];
                for (int v = 0; v < a.NV; v++) {
                    float f4[4], wf[4], da[4];
                    awg_ld4(fj + 4 * v, f4);
#pragma unroll
                    for (int c = 0; c < 4; c++) wf[c] = w[G == 1 ? 0 : c / SG] * f4[c];
                    awg_da(a, b, (size_t)i * a.C + me.c0 + 4 * v, sc, wf, da);
#pragma unroll
                    for (int c = 0; c < 4; c++) dw[G == 1 ? 0 : c / SG] += da[c] * f4[c];
                }
#pragma unroll
                for (int g = 0; g < G; g++) gn[g] += sm ? w[g] * (dw[g] - b.D[(size_t)i * a.M + me.m0 + g]) : dw[g];
            }
#pragma unroll
            for (int g = 0; g < G; g++) grad_neighbor[(size_t)j * a.M + me.m0 + g] = gn[g];
        }
        if (!grad_value) continue;
        for (int v0 = 0; v0 < a.NV; v0 += VB) {                        // grad_features_value[j, c] = sum over j's pairs of da w
            float acc[VB][4], f4[VB][4];
#pragma unroll
            for (int u = 0; u < VB; u++) {
#pragma unroll
                for (int c = 0; c < 4; c++) { acc[u][c] = 0.f; f4[u][c] = 0.f; }
                if (a.red == AWG_MAX && v0 + u < a.NV) awg_ld4(fj + 4 * (v0 + u), f4[u]);
            }
            for (int e = e0; e < e1; e++) {
                const int i = (int)cbl_fastdiv((unsigned)inv_src[e], dvK);
                const AwgQuery Q = awg_query(a, i);
                float cen[G], r[3], y[G], w[G];
                awg_row<G>(a.cen, a.M, me.m0, a.idx[(size_t)i * a.K], a.n0, cen);
                awg_eval<G>(t, a.inv_radius, sx, sy, sz, Q, cen, nb, r, y);
#pragma unroll
                for (int g = 0; g < G; g++) w[g] = awg_weight(a.softmax, true, y[g], sm ? b.lse[(size_t)i * a.M + me.m0 + g] : 0.f);
                const float sc = b.inv_nn[i];
#pragma unroll
                for (int u = 0; u < VB; u++) {
                    if (v0 + u >= a.NV) continue;
                    float wf[4], da[4];
#pragma unroll
                    for (int c = 0; c < 4; c++) wf[c] = w[G == 1 ? 0 : c / SG] * f4[u][c];
                    awg_da(a, b, (size_t)i * a.C + me.c0 + 4 * (v0 + u), sc, wf, da);
#pragma unroll
                    for (int c = 0; c < 4; c++) acc[u][c] += da[c] * w[G == 1 ? 0 : c / SG];
                }
            }
#pragma unroll
            for (int u = 0; u < VB; u++)
                if (v0 + u < a.NV) awg_st4(grad_value + (size_t)j * a.C + me.c0 + 4 * (v0 + u), acc[u]);
        }
    }
}

// ---------------------------------------------------------------- host side
int awg_check(int n, int n0, int K, int C, int M, float radius, int softmax, int reduction)
{
    if (n < 0 || n0 < 0 || K <= 0 || C <= 0 || M <= 0 || !(radius > 0.f)) return CBL_ERR_BAD_ARG;
    if (softmax < 0 || softmax > AWG_SM_UNMASK || reduction < 0 || reduction > AWG_MAX) return CBL_ERR_BAD_ARG;
    if (K > AWG_KMAX || C % 4 != 0 || C > AWG_CMAX || C % M != 0) return CBL_ERR_UNSUPPORTED;
    const int S = C / M;
    if (!(S == 1 || S == 2 || S == 4 || S % 4 == 0)) return CBL_ERR_UNSUPPORTED;
    return CBL_OK;
}

inline size_t awg_up(size_t b) { return (b + 255) & ~(size_t)255; }
struct AwgSpace { size_t partial, lse, D, inv_nn, ties, total; };
inline AwgSpace awg_space(int n, int C, int M)
{
    const size_t rows = (size_t)(n > 0 ? n : 0);
    AwgSpace s;
    s.partial = 0;
    s.lse = awg_up(sizeof(double) * (size_t)AWG_MAX_BLOCKS * 4 * M);
    s.D = s.lse + awg_up(sizeof(float) * rows * M);
    s.inv_nn = s.D + awg_up(sizeof(float) * rows * M);
    s.ties = s.inv_nn + awg_up(sizeof(float) * rows);
    s.total = s.ties + awg_up(sizeof(float) * rows * C);
    return s;
}

inline AwgArgs awg_args(int n, int n0, int K, int C, int M, const float* q, const float* s, const int* idx, const float* f, const float* cen, const float* nbr,
                        const float* wp, const float* bias, float radius, int softmax, int red, const int* padding_num)
{
    AwgArgs a;
    a.n = n; a.n0 = n0; a.K = K; a.C = C; a.M = M; a.S = C / M;
    a.NV = (a.S > 4 ? a.S : 4) / 4; a.Lr = C / (4 * a.NV);
    const int ncb = (a.Lr + AWG_BLOCK - 1) / AWG_BLOCK;
    a.Lb = (a.Lr + ncb - 1) / ncb; a.tpb = AWG_BLOCK / a.Lb;
    a.q = q; a.s = s; a.idx = idx; a.f = f; a.cen = cen; a.nbr = nbr; a.wp = wp; a.bias = bias; a.inv_radius = 1.0f / radius;
    a.softmax = softmax; a.red = red; a.padding_num = padding_num;
    return a;
}
inline dim3 awg_grid(const AwgArgs& a, int rows, int cap)
{
    return dim3(cbl_grid_for(((long long)rows + a.tpb - 1) / a.tpb, 1, cap), (unsigned)((a.Lr + a.Lb - 1) / a.Lb));
}
inline int awg_groups_per_lane(int S) { return S >= 4 ? 1 : 4 / S; }

}  // namespace

#define AWG_LAUNCH(kernel, a, grid, st, ...)                                                                                        \
    do {                                                                                                                            \
        const int G_ = awg_groups_per_lane((a).S);                                                                                  \
        if (G_ == 4) hipLaunchKernelGGL(kernel<4>, grid, dim3(AWG_BLOCK), 0, st, __VA_ARGS__);                                      \
        else if (G_ == 2) hipLaunchKernelGGL(kernel<2>, grid, dim3(AWG_BLOCK), 0, st, __VA_ARGS__);                                 \
        else hipLaunchKernelGGL(kernel<1>, grid, dim3(AWG_BLOCK), 0, st, __VA_ARGS__);                                              \
    } while (0)

CBL_EXPORT size_t cbl_adaptive_weight_general_workspace_bytes(int n, int n0, int K, int C, int M)
{
    if (awg_check(n, n0, K, C, M, 1.f, 0, 0) != CBL_OK) return 0;
    return awg_space(n, C, M).total + 256;
}

CBL_EXPORT int cbl_adaptive_weight_general_forward(int n, int n0, int K, int C, int M, const float* query_points, const float* support_points,
                                                   const int* neighbors_indices, const float* features, const float* center_term, const float* neighbor_term,
                                                   const float* w_pos, const float* bias, float radius, int softmax, int reduction, const int* padding_num,
                                                   float* out, void* workspace, size_t workspace_bytes, void* stream)
{
    (void)workspace; (void)workspace_bytes;                           // (the forward pass keeps its rows in registers)
    const int rc = awg_check(n, n0, K, C, M, radius, softmax, reduction);
    if (rc) return rc;
    if (n == 0) return CBL_OK;
    if (!query_points || !support_points || !neighbors_indices || !features || !bias || !out || (reduction == AWG_MEAN && !padding_num)) return CBL_ERR_BAD_ARG;
    if (!cbl_host_aligned16(features) || !cbl_host_aligned16(out)) return CBL_ERR_UNSUPPORTED;
    hipStream_t st = cbl_stream(stream);
    const AwgArgs a = awg_args(n, n0, K, C, M, query_points, support_points, neighbors_indices, features, center_term, neighbor_term, w_pos, bias, radius,
                               softmax, reduction, padding_num);
    AWG_LAUNCH(awg_forward_kernel, a, awg_grid(a, n, 8192), st, a, out);
    return cbl_status();
}

CBL_EXPORT int cbl_adaptive_weight_general_backward_csr(int n, int n0, int K, int C, int M, const float* query_points, const float* support_points,
                                                        const int* neighbors_indices, const float* features, const float* center_term,
                                                        const float* neighbor_term, const float* w_pos, const float* bias, float radius, int softmax,
                                                        int reduction, const int* padding_num, const float* out, const float* grad_out,
                                                        const int* order_dst, const int* inv_start, const int* inv_src,
                                                        float* grad_features_value, float* grad_center, float* grad_neighbor, float* grad_w_pos, float* grad_bias,
                                                        void* workspace, size_t workspace_bytes, void* stream)
{
    const int rc = awg_check(n, n0, K, C, M, radius, softmax, reduction);
    if (rc) return rc;
    if (!grad_features_value && !grad_center && !grad_neighbor && !grad_w_pos && !grad_bias) return CBL_OK;
    if (n > 0 && (!query_points || !support_points || !neighbors_indices || !features || !bias || !grad_out || (reduction == AWG_MEAN && !padding_num) ||
                  (reduction == AWG_MAX && !out))) return CBL_ERR_BAD_ARG;
    const bool table = (grad_features_value || grad_neighbor) && n0 > 0;
    if (table && (!inv_start || !inv_src || !support_points || !features)) return CBL_ERR_BAD_ARG;
    if (!workspace || !cbl_host_aligned16(workspace)) return CBL_ERR_BAD_ARG;
    if (workspace_bytes < cbl_adaptive_weight_general_workspace_bytes(n, n0, K, C, M)) return CBL_ERR_WORKSPACE;
    if (!cbl_host_aligned16(features) || !cbl_host_aligned16(out) || !cbl_host_aligned16(grad_out) || !cbl_host_aligned16(grad_features_value))
        return CBL_ERR_UNSUPPORTED;
    hipStream_t st = cbl_stream(stream);
    if (n == 0) {                                                    // no pair: every sum is empty
        if (grad_features_value && n0 > 0) (void)hipMemsetAsync(grad_features_value, 0, sizeof(float) * (size_t)n0 * C, st);
        if (grad_neighbor && n0 > 0) (void)hipMemsetAsync(grad_neighbor, 0, sizeof(float) * (size_t)n0 * M, st);
        if (grad_w_pos) (void)hipMemsetAsync(grad_w_pos, 0, sizeof(float) * 3 * (size_t)M, st);
        if (grad_bias) (void)hipMemsetAsync(grad_bias, 0, sizeof(float) * (size_t)M, st);
        return cbl_status();
    }
    const AwgSpace sp = awg_space(n, C, M);
    char* base = reinterpret_cast<char*>(workspace);
    double* partial = reinterpret_cast<double*>(base + sp.partial);
    const AwgArgs a = awg_args(n, n0, K, C, M, query_points, support_points, neighbors_indices, features, center_term, neighbor_term, w_pos, bias, radius,
                               softmax, reduction, padding_num);
    AwgBwd b;
    b.go = grad_out; b.out = out;
    b.lse = reinterpret_cast<float*>(base + sp.lse); b.D = reinterpret_cast<float*>(base + sp.D);
    b.inv_nn = reinterpret_cast<float*>(base + sp.inv_nn); b.ties = reinterpret_cast<float*>(base + sp.ties);
    const bool sums = grad_w_pos || grad_bias;
    const dim3 gq = awg_grid(a, n, AWG_MAX_BLOCKS);
    AWG_LAUNCH(awg_bwd_query_kernel, a, gq, st, a, b, grad_center, sums ? partial : (double*)nullptr);
    if (sums)
        hipLaunchKernelGGL(awg_finalize_kernel, dim3(cbl_div_up(M, AWG_FIN_M)), dim3(256), 0, st, M, (int)gq.x, (const double*)partial, grad_w_pos, grad_bias);
    if (table) {
        const dim3 gt = awg_grid(a, n0, 8192);
        AWG_LAUNCH(awg_bwd_target_kernel, a, gt, st, a, b, cbl_fastdiv_make((unsigned)K), order_dst, inv_start, inv_src, grad_neighbor, grad_features_value);
    }
    return cbl_status();
}

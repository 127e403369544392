// a14: PointWiseMLP — local aggregation by one shared FC layer + batch norm + activation per (query, neighbour) pair, reduced over the K neighbours.
// Replaces the TF1 op chain of PointWiseMLP  tensorflow/models/local_aggregation_operators.py:503-617 with fc_num 1 (batch_conv1d_1x1 `fc_1`,
// basic_operators.py:243-289; batch norm :134-152).  The graph form materialises an (n, K, D_in) concatenation and (n, K, C_out) activations; one FC
// layer is linear in the concatenated blocks, so for the pair (i, k) with neighbour j = idx[i, k] every local_input_feature reduces to
//     y[i,k,:] = ((s_j - q_i) / radius) @ W_p  +  Cen[idx[i,0]]  +  Nbr[j]          Cen = features @ (W_fi - W_df),  Nbr = features @ (W_df + W_fj)
// (two per-point (n0, C_out) products made by the caller; shadow rows are zero, the shadow point is the origin), followed by
//     out[i,:] = reduce_k  mask[i,k] * act( gamma * (y - mean) * invstd + beta )      statistics over all n*K pairs, shadow pairs included.
// Every pass RECOMPUTES y from the gathered Nbr row, the query's Cen row and a 3 x C_out product; nothing of shape (n, K, .) exists in memory.
//
// MI355X mapping.  Query-side passes: lane = 4 consecutive channels of one query, the C_out/4 lanes of a query next to each other (a neighbour's row is one
// contiguous burst), 256 / (C_out/4) queries per workgroup trip; a lane keeps its channels for the whole launch, so w_pos / mean / invstd / gamma / beta sit
// in registers.  Target-side pass (grad_neighbor): the same layout over the targets of the transposed neighbour table, written, not accumulated.
//   forward   F1 (batch statistics only): sum y, sum y^2 per channel — fp64 per lane, per-workgroup partials in the workspace, fixed-order finalize
//             F2: normalise, activate, mask, reduce over K -> out
//   backward  B1: sum dz (= d beta), sum dz * xhat (= d gamma); 'max': the per-(i, c) tie count
//             B2: dy -> grad_center (n, C_out) rows = sum_k dy, grad_w_pos = sum dp^T dy (per-workgroup partials, fixed-order finalize)
//             B3: grad_neighbor[j] = sum over j's segment of the transposed table of dy, recomputed from per-query rows
// No float atomics: partial sums are combined in a fixed order (fp64), every output is stored once.  Bound by the gathered rows (L2 / Infinity Cache):
// algorithmic bytes per query-side pass 4 n K C_out (Nbr rows) + 4 n C_out (Cen row) + 4 n K + 12 (n K + n), B3 three to five rows per pair.
#include "cbl_common.h"

namespace {

enum { PW_BN_NONE = 0, PW_BN_BATCH = 1, PW_BN_MOVING = 2 };
enum { PW_ACT_NONE = 0, PW_ACT_RELU = 1, PW_ACT_LEAKY = 2 };
enum { PW_SUM = 0, PW_MEAN = 1, PW_MAX = 2 };
enum { PW_FIN_STATS = 0, PW_FIN_BN_BWD = 1, PW_FIN_WPOS = 2 };
constexpr int PW_KMAX = 128, PW_CMAX = 1024, PW_BLOCK = 256, PW_MAX_BLOCKS = 1024;
constexpr int PW_FIN_CH = 8, PW_FIN_SLICES = 32;                   // the finalize workgroup: 8 channels x 32 slices of the partials

struct PwArgs {
    int n, n0, K, C, L, tpb;                   // L = C / 4 lanes per row, tpb = 256 / L rows per workgroup trip
    const float* q; const float* s; const int* idx;
    const float* cen; const float* nbr; const float* wp;
    float inv_radius;
    int bn_mode, act, red;
    const float* gamma; const float* beta; const float* mean; const float* invstd;
    const int* padding_num;
};
struct PwBwd {                                  // what the backward passes read on top
    const float* go; const float* out; const float* coef; const float* inv_nn;
    float* ties;
};

struct PwLane { float w[3][4], mu[4], is[4], ga[4], be[4], k0[4], k1[4]; };     // a lane's four channels
struct PwQuery { float qx, qy, qz, cen[4]; };
struct PwPair { float rx, ry, rz, xh[4], z[4]; };

__device__ __forceinline__ void pw_ld4(const float* p, float (&v)[4])
{
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void pw_st4(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void pw_set4(float (&v)[4], float x) { v[0] = v[1] = v[2] = v[3] = x; }

__device__ __forceinline__ PwLane pw_lane(const PwArgs& a, int c0, const float* coef)
{
    PwLane t;
    for (int d = 0; d < 3; d++) { if (a.wp) pw_ld4(a.wp + (size_t)d * a.C + c0, t.w[d]); else pw_set4(t.w[d], 0.f); }
    const bool bn = a.bn_mode != PW_BN_NONE;
    if (bn) { pw_ld4(a.mean + c0, t.mu); pw_ld4(a.invstd + c0, t.is); } else { pw_set4(t.mu, 0.f); pw_set4(t.is, 1.f); }
    if (bn && a.gamma) pw_ld4(a.gamma + c0, t.ga); else pw_set4(t.ga, 1.f);
    if (bn && a.beta) pw_ld4(a.beta + c0, t.be); else pw_set4(t.be, 0.f);
    if (coef && a.bn_mode == PW_BN_BATCH) { pw_ld4(coef + c0, t.k0); pw_ld4(coef + a.C + c0, t.k1); } else { pw_set4(t.k0, 0.f); pw_set4(t.k1, 0.f); }
    return t;
}

__device__ __forceinline__ bool pw_real(int id, int n0) { return id >= 0 && id < n0; }

// the centre row of query i: shadow_features[idx[i, 0]] folded through (W_fi - W_df)  (:556) — zero when that entry is the shadow row
__device__ __forceinline__ void pw_center(const PwArgs& a, int c0, int i, float (&cen)[4])
{
    pw_set4(cen, 0.f);
    if (a.cen) {
        const int cid = a.idx[(size_t)i * a.K];
        if (pw_real(cid, a.n0)) pw_ld4(a.cen + (size_t)cid * a.C + c0, cen);
    }
}
__device__ __forceinline__ PwQuery pw_query(const PwArgs& a, int c0, int i)
{
    PwQuery Q;
    Q.qx = a.q[3 * (size_t)i]; Q.qy = a.q[3 * (size_t)i + 1]; Q.qz = a.q[3 * (size_t)i + 2];
    pw_center(a, c0, i, Q.cen);
    return Q;
}

// y, xhat and z of one pair from its pieces — ONE expression for every pass: 'max' compares a recomputed activation with the forward's stored maximum
__device__ __forceinline__ void pw_eval(const PwLane& t, float inv_radius, float sx, float sy, float sz, float qx, float qy, float qz, const float (&cen)[4],
                                        const float (&nb)[4], PwPair& P, float (&y)[4])
{
    P.rx = (sx - qx) * inv_radius; P.ry = (sy - qy) * inv_radius; P.rz = (sz - qz) * inv_radius;         // :563-564
#pragma unroll
    for (int v = 0; v < 4; v++) {
        y[v] = (((P.rx * t.w[0][v] + P.ry * t.w[1][v]) + P.rz * t.w[2][v]) + cen[v]) + nb[v];
        P.xh[v] = (y[v] - t.mu[v]) * t.is[v];
        P.z[v] = P.xh[v] * t.ga[v] + t.be[v];
    }
}
// the pair (query Q, neighbour id) seen from the query: shadow neighbour = zero row at the origin (:552-561)
__device__ __forceinline__ bool pw_pair(const PwArgs& a, const PwLane& t, int c0, int id, const PwQuery& Q, PwPair& P, float (&y)[4])
{
    const bool real = pw_real(id, a.n0);
    float sx = 0.f, sy = 0.f, sz = 0.f, nb[4] = {0.f, 0.f, 0.f, 0.f};
    if (real) {
        sx = a.s[3 * (size_t)id]; sy = a.s[3 * (size_t)id + 1]; sz = a.s[3 * (size_t)id + 2];
        pw_ld4(a.nbr + (size_t)id * a.C + c0, nb);
    }
    pw_eval(t, a.inv_radius, sx, sy, sz, Q.qx, Q.qy, Q.qz, Q.cen, nb, P, y);
    return real;
}

__device__ __forceinline__ float pw_act(float z, int act)         // basic_operators.py:285-289: any other string is the identity
{
    return act == PW_ACT_RELU ? (z > 0.f ? z : 0.f) : act == PW_ACT_LEAKY ? (z > 0.f ? z : 0.2f * z) : z;
}
__device__ __forceinline__ float pw_dact(float z, int act)
{
    return act == PW_ACT_RELU ? (z > 0.f ? 1.f : 0.f) : act == PW_ACT_LEAKY ? (z > 0.f ? 1.f : 0.2f) : 1.f;
}
// gradient at z of a pair: g = the query's gradient row already divided by nn ('mean') or by the tie count ('max'); m = the row's maximum ('max')
__device__ __forceinline__ float pw_dz(bool real, float z, float g, float m, int act, int red)
{
    if (!real) return 0.f;                                           // the mask sits behind the activation (:601): a shadow pair passes nothing on
    if (red == PW_MAX && !(pw_act(z, act) == m)) return 0.f;
    return pw_dact(z, act) * g;
}
// gradient at y through the batch norm; bn_mode 1 couples all pairs (non-zero on shadow pairs too)
__device__ __forceinline__ float pw_dy(const PwLane& t, int v, int bn_mode, float dz, float xh)
{
    if (bn_mode == PW_BN_BATCH) return (t.ga[v] * t.is[v]) * ((dz - t.k0[v]) - xh * t.k1[v]);
    if (bn_mode == PW_BN_MOVING) return (t.ga[v] * t.is[v]) * dz;
    return dz;
}

// per-lane sums acc[r][v] (r < V) of the lanes that share a channel quad -> partial[(block * V + r) * C + c], in the fixed order of the rows of a workgroup
template <int V>
__device__ __forceinline__ void pw_block_partial(const PwArgs& a, bool live, int ts, int cl, const double (&acc)[V][4], double (*red)[PW_BLOCK][4], double* partial)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int r = 0; r < V; r++)
#pragma unroll
        for (int v = 0; v < 4; v++) red[r][tid][v] = acc[r][v];
    __syncthreads();
    if (live && ts == 0) {
        for (int r = 0; r < V; r++)
            for (int v = 0; v < 4; v++) {
                double sum = 0.0;
                for (int s = 0; s < a.tpb; s++) sum += red[r][s * a.L + cl][v];
                partial[((size_t)blockIdx.x * V + r) * a.C + 4 * cl + v] = sum;
            }
    }
}

// ---------------------------------------------------------------- F1: batch statistics of y over all n*K pairs
// fp64 per lane: with features of mean 8 |mean y| is many standard deviations, where fp32 sums of y^2 leave the variance no digits
__global__ __launch_bounds__(PW_BLOCK) void pw_stats_kernel(PwArgs a, double* __restrict__ partial)
{
    __shared__ double red[2][PW_BLOCK][4];
    const int ts = threadIdx.x / a.L, cl = threadIdx.x - ts * a.L, c0 = 4 * cl;
    const bool live = ts < a.tpb;
    double acc[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    if (live) {
        PwArgs b = a; b.bn_mode = PW_BN_NONE;                        // (no statistics yet)
        const PwLane t = pw_lane(b, c0, nullptr);
        const int ntrips = (a.n + a.tpb - 1) / a.tpb;
        for (int trip = blockIdx.x; trip < ntrips; trip += gridDim.x) {
            const int i = trip * a.tpb + ts;
            if (i >= a.n) continue;
            const PwQuery Q = pw_query(a, c0, i);
            const int* __restrict__ row = a.idx + (size_t)i * a.K;
#pragma unroll 2
            for (int k = 0; k < a.K; k++) {
                PwPair P; float y[4];
                pw_pair(a, t, c0, row[k], Q, P, y);
#pragma unroll
                for (int v = 0; v < 4; v++) { const double d = (double)y[v]; acc[0][v] += d; acc[1][v] += d * d; }
            }
        }
    }
    pw_block_partial<2>(a, live, ts, cl, acc, red, partial);
}

// sums of the per-workgroup partials: 8 channels per workgroup, lane (channel, slice js) adds every 32nd partial, slices combined through LDS (fp64)
__global__ __launch_bounds__(256) void pw_finalize_kernel(int what, int C, int nblocks, const double* __restrict__ partial, double N, float eps, float momentum,
                                                          float* __restrict__ moving_mean, float* __restrict__ moving_var,
                                                          float* __restrict__ o0, float* __restrict__ o1, float* __restrict__ coef)
{
    __shared__ double red[PW_FIN_SLICES][PW_FIN_CH][3];
    const int V = what == PW_FIN_WPOS ? 3 : 2;
    const int cs = threadIdx.x % PW_FIN_CH, js = threadIdx.x / PW_FIN_CH, c = blockIdx.x * PW_FIN_CH + cs;
    double s[3] = {0.0, 0.0, 0.0};
    if (c < C) {
        // (independent loads kept in flight: one lane per channel walking its partials one by one is a chain of dependent-latency loads)
#pragma unroll 4
        for (int b = js; b < nblocks; b += PW_FIN_SLICES) {
            s[0] += partial[((size_t)b * V + 0) * C + c];
            s[1] += partial[((size_t)b * V + 1) * C + c];
            if (V == 3) s[2] += partial[((size_t)b * V + 2) * C + c];
        }
    }
    for (int r = 0; r < 3; r++) red[js][cs][r] = s[r];
    __syncthreads();
    if (js != 0 || c >= C) return;
    double t[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < PW_FIN_SLICES; j++) for (int r = 0; r < 3; r++) t[r] += red[j][cs][r];
    if (what == PW_FIN_STATS) {
        const double mu = t[0] / N;
        double var = t[1] / N - mu * mu;                              // biased, as tf.nn.moments
        if (var < 0.0) var = 0.0;
        o0[c] = (float)mu;
        o1[c] = (float)(1.0 / sqrt(var + (double)eps));
        // tf.layers.batch_normalization: moving = moving * momentum + batch * (1 - momentum), with the BIASED variance (not torch's unbiased one)
        if (moving_mean) moving_mean[c] = moving_mean[c] * momentum + (float)mu * (1.f - momentum);
        if (moving_var) moving_var[c] = moving_var[c] * momentum + (float)var * (1.f - momentum);
    } else if (what == PW_FIN_BN_BWD) {
        if (o0) o0[c] = (float)t[1];                                  // grad_gamma = sum dz * xhat
        if (o1) o1[c] = (float)t[0];                                  // grad_beta = sum dz
        coef[c] = (float)(t[0] / N); coef[C + c] = (float)(t[1] / N);
    } else {
        for (int r = 0; r < 3; r++) o0[(size_t)r * C + c] = (float)t[r];
    }
}

// bn_mode 2: the statistics are the moving ones
__global__ __launch_bounds__(256) void pw_moving_kernel(int C, const float* __restrict__ moving_mean, const float* __restrict__ moving_var, float eps,
                                                        float* __restrict__ mean, float* __restrict__ invstd)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < C) { mean[c] = moving_mean[c]; invstd[c] = (float)(1.0 / sqrt((double)moving_var[c] + (double)eps)); }
}

// ---------------------------------------------------------------- F2: normalise, activate, mask, reduce over K
__global__ __launch_bounds__(PW_BLOCK) void pw_forward_kernel(PwArgs a, float* __restrict__ out)
{
    const int ts = threadIdx.x / a.L, cl = threadIdx.x - ts * a.L, c0 = 4 * cl;
    if (ts >= a.tpb) return;
    const PwLane t = pw_lane(a, c0, nullptr);
    const int pad = (a.red == PW_MEAN) ? *a.padding_num : 0;
    const int ntrips = (a.n + a.tpb - 1) / a.tpb;
    for (int trip = blockIdx.x; trip < ntrips; trip += gridDim.x) {
        const int i = trip * a.tpb + ts;
        if (i >= a.n) continue;
        const PwQuery Q = pw_query(a, c0, i);
        const int* __restrict__ row = a.idx + (size_t)i * a.K;
        float acc[4];
        pw_set4(acc, a.red == PW_MAX ? -INFINITY : 0.f);
        int cnt = 0;
#pragma unroll 2
        for (int k = 0; k < a.K; k++) {
            const int id = row[k];
            cnt += (id < pad) ? 1 : 0;
            PwPair P; float y[4];
            const bool real = pw_pair(a, t, c0, id, Q, P, y);
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const float av = real ? pw_act(P.z[v], a.act) : 0.f;     // activation * mask (:601): a shadow pair is 0, also under 'max'
                if (a.red == PW_MAX) acc[v] = av > acc[v] ? av : acc[v]; else acc[v] += av;
            }
        }
        if (a.red == PW_MEAN) {
            const float nn = (float)cnt + 1e-5f;                      // :609-613
#pragma unroll
            for (int v = 0; v < 4; v++) acc[v] = acc[v] / nn;
        }
        pw_st4(out + (size_t)i * a.C + c0, acc);
    }
}

// ---------------------------------------------------------------- backward
__global__ __launch_bounds__(256) void pw_inv_count_kernel(int n, int K, const int* __restrict__ idx, const int* __restrict__ padding_num, int red,
                                                           float* __restrict__ inv_nn)
{
    const int pad = (red == PW_MEAN) ? *padding_num : 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        int cnt = 0;
        if (red == PW_MEAN)
            for (int k = 0; k < K; k++) cnt += idx[(size_t)i * K + k] < pad ? 1 : 0;
        inv_nn[i] = (red == PW_MEAN) ? 1.0f / ((float)cnt + 1e-5f) : 1.0f;
    }
}

// the gradient row of query i as the pairs take it: g = grad_out / nn ('mean'), grad_out / ties ('max', with m = the row's maximum)
__device__ __forceinline__ void pw_grad_row(const PwArgs& a, const PwBwd& w, int c0, int i, float (&g)[4], float (&m)[4])
{
    pw_ld4(w.go + (size_t)i * a.C + c0, g);
    pw_set4(m, 0.f);
    if (a.red == PW_MAX) {
        float tc[4];
        pw_ld4(w.out + (size_t)i * a.C + c0, m);
        pw_ld4(w.ties + (size_t)i * a.C + c0, tc);
#pragma unroll
        for (int v = 0; v < 4; v++) g[v] = tc[v] > 0.f ? g[v] / tc[v] : 0.f;
    } else {
        const float sc = w.inv_nn[i];
#pragma unroll
        for (int v = 0; v < 4; v++) g[v] = g[v] * sc;
    }
}

// B1: 'max': ties[i, c] = #{k : activation * mask == out[i, c]}  (tf.reduce_max shares the gradient among them; shadow pairs, value 0, count);
//     SUMS: partial sums of dz and dz * xhat
__global__ __launch_bounds__(PW_BLOCK) void pw_bwd_sums_kernel(PwArgs a, PwBwd w, int sums, double* __restrict__ partial)
{
    __shared__ double red[2][PW_BLOCK][4];
    const int ts = threadIdx.x / a.L, cl = threadIdx.x - ts * a.L, c0 = 4 * cl;
    const bool live = ts < a.tpb;
    double acc[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    if (live) {
        const PwLane t = pw_lane(a, c0, nullptr);
        const int ntrips = (a.n + a.tpb - 1) / a.tpb;
        for (int trip = blockIdx.x; trip < ntrips; trip += gridDim.x) {
            const int i = trip * a.tpb + ts;
            if (i >= a.n) continue;
            const PwQuery Q = pw_query(a, c0, i);
            const int* __restrict__ row = a.idx + (size_t)i * a.K;
            float g[4], m[4], tc[4] = {0.f, 0.f, 0.f, 0.f}, s0[4] = {0.f, 0.f, 0.f, 0.f}, s1[4] = {0.f, 0.f, 0.f, 0.f};
            if (a.red == PW_MAX) { pw_ld4(w.go + (size_t)i * a.C + c0, g); pw_ld4(w.out + (size_t)i * a.C + c0, m); }
            else pw_grad_row(a, w, c0, i, g, m);
#pragma unroll 2
            for (int k = 0; k < a.K; k++) {
                PwPair P; float y[4];
                const bool real = pw_pair(a, t, c0, row[k], Q, P, y);
#pragma unroll
                for (int v = 0; v < 4; v++) {
                    if (a.red == PW_MAX) {
                        // one walk for both: the row's gradient is grad_out / ties on every pair that attains the maximum, so the sums are taken without
                        // that factor and scaled once the count is known
                        const bool hit = (real ? pw_act(P.z[v], a.act) : 0.f) == m[v];
                        tc[v] += hit ? 1.f : 0.f;
                        const float d = (hit && real) ? pw_dact(P.z[v], a.act) : 0.f;
                        s0[v] += d; s1[v] += d * P.xh[v];
                    } else {
                        const float dz = pw_dz(real, P.z[v], g[v], m[v], a.act, a.red);
                        s0[v] += dz; s1[v] += dz * P.xh[v];
                    }
                }
            }
            if (a.red == PW_MAX) {
                pw_st4(w.ties + (size_t)i * a.C + c0, tc);
#pragma unroll
                for (int v = 0; v < 4; v++) { const float sc = tc[v] > 0.f ? g[v] / tc[v] : 0.f; s0[v] *= sc; s1[v] *= sc; }
            }
#pragma unroll
            for (int v = 0; v < 4; v++) { acc[0][v] += (double)s0[v]; acc[1][v] += (double)s1[v]; }
        }
    }
    if (sums) pw_block_partial<2>(a, live, ts, cl, acc, red, partial);
}

// B2: grad_center[i, :] = sum_k dy[i, k, :] (every pair, shadow pairs included: their centre row is the query's), partial sums of dp^T dy
__global__ __launch_bounds__(PW_BLOCK) void pw_bwd_query_kernel(PwArgs a, PwBwd w, float* __restrict__ grad_center, int wpos, double* __restrict__ partial)
{
    __shared__ double red[3][PW_BLOCK][4];
    const int ts = threadIdx.x / a.L, cl = threadIdx.x - ts * a.L, c0 = 4 * cl;
    const bool live = ts < a.tpb;
    double acc[3][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    if (live) {
        const PwLane t = pw_lane(a, c0, w.coef);
        const int ntrips = (a.n + a.tpb - 1) / a.tpb;
        for (int trip = blockIdx.x; trip < ntrips; trip += gridDim.x) {
            const int i = trip * a.tpb + ts;
            if (i >= a.n) continue;
            const PwQuery Q = pw_query(a, c0, i);
            const int* __restrict__ row = a.idx + (size_t)i * a.K;
            float g[4], m[4], gc[4] = {0.f, 0.f, 0.f, 0.f}, gw[3][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            pw_grad_row(a, w, c0, i, g, m);
#pragma unroll 2
            for (int k = 0; k < a.K; k++) {
                PwPair P; float y[4];
                const bool real = pw_pair(a, t, c0, row[k], Q, P, y);
#pragma unroll
                for (int v = 0; v < 4; v++) {
                    const float dy = pw_dy(t, v, a.bn_mode, pw_dz(real, P.z[v], g[v], m[v], a.act, a.red), P.xh[v]);
                    gc[v] += dy;
                    gw[0][v] += P.rx * dy; gw[1][v] += P.ry * dy; gw[2][v] += P.rz * dy;
                }
            }
            if (grad_center) pw_st4(grad_center + (size_t)i * a.C + c0, gc);
#pragma unroll
            for (int d = 0; d < 3; d++)
#pragma unroll
                for (int v = 0; v < 4; v++) acc[d][v] += (double)gw[d][v];
        }
    }
    if (wpos) pw_block_partial<3>(a, live, ts, cl, acc, red, partial);
}

// B3: grad_neighbor[j, :] = sum over the pairs p = i*K + k of j's segment (ascending) of dy[p, :], dy recomputed from the rows of query i.
// A shadow pair is in no segment (its neighbour row is a constant zero).
__global__ __launch_bounds__(PW_BLOCK) void pw_bwd_target_kernel(PwArgs a, PwBwd w, CblFastDiv dvK, const int* __restrict__ order, const int* __restrict__ inv_start,
                                                                 const int* __restrict__ inv_src, float* __restrict__ grad_neighbor)
{
    const int ts = threadIdx.x / a.L, cl = threadIdx.x - ts * a.L, c0 = 4 * cl;
    if (ts >= a.tpb) return;
    const PwLane t = pw_lane(a, c0, w.coef);
    // what a pair's dy needs beyond its gradient row: nothing when there is neither an activation, nor batch statistics, nor a maximum to compare with
    const bool need_z = a.act != PW_ACT_NONE || a.bn_mode == PW_BN_BATCH || a.red == PW_MAX;
    const int ntrips = (a.n0 + a.tpb - 1) / a.tpb;
    for (int trip = blockIdx.x; trip < ntrips; trip += gridDim.x) {
        const int tr = trip * a.tpb + ts;
        if (tr >= a.n0) continue;
        const int j = order ? order[tr] : tr;
        const int e0 = inv_start[tr], e1 = inv_start[tr + 1];
        const float sx = a.s[3 * (size_t)j], sy = a.s[3 * (size_t)j + 1], sz = a.s[3 * (size_t)j + 2];
        float nb[4], acc[4] = {0.f, 0.f, 0.f, 0.f};
        pw_ld4(a.nbr + (size_t)j * a.C + c0, nb);
#pragma unroll 2
        for (int e = e0; e < e1; e++) {
            const int i = (int)cbl_fastdiv((unsigned)inv_src[e], dvK);
            float g[4], m[4];
            pw_grad_row(a, w, c0, i, g, m);
            PwPair P;
            pw_set4(P.xh, 0.f); pw_set4(P.z, 1.f);
            if (need_z) {
                float cen[4], y[4];
                pw_center(a, c0, i, cen);
                pw_eval(t, a.inv_radius, sx, sy, sz, a.q[3 * (size_t)i], a.q[3 * (size_t)i + 1], a.q[3 * (size_t)i + 2], cen, nb, P, y);
            }
#pragma unroll
            for (int v = 0; v < 4; v++) acc[v] += pw_dy(t, v, a.bn_mode, pw_dz(true, P.z[v], g[v], m[v], a.act, a.red), P.xh[v]);
        }
        pw_st4(grad_neighbor + (size_t)j * a.C + c0, acc);
    }
}

// ---------------------------------------------------------------- host side
int pw_check(int n, int n0, int K, int C, float radius, int bn_mode, int activation, int reduction)
{
    if (n < 0 || n0 < 0 || K <= 0 || C <= 0 || !(radius > 0.f)) return CBL_ERR_BAD_ARG;
    if (bn_mode < 0 || bn_mode > PW_BN_MOVING || activation < 0 || activation > PW_ACT_LEAKY || reduction < 0 || reduction > PW_MAX) return CBL_ERR_BAD_ARG;
    if (K > PW_KMAX || C % 4 != 0 || C > PW_CMAX) return CBL_ERR_UNSUPPORTED;
    return CBL_OK;
}

inline size_t pw_up(size_t b) { return (b + 255) & ~(size_t)255; }
struct PwSpace { size_t partial, coef, inv_nn, ties, total; };
inline PwSpace pw_space(int n, int C)
{
    PwSpace s;
    s.partial = 0;
    s.coef = pw_up(sizeof(double) * (size_t)PW_MAX_BLOCKS * 3 * C);
    s.inv_nn = s.coef + pw_up(sizeof(float) * 2 * (size_t)C);
    s.ties = s.inv_nn + pw_up(sizeof(float) * (size_t)(n > 0 ? n : 0));
    s.total = s.ties + pw_up(sizeof(float) * (size_t)(n > 0 ? n : 0) * C);
    return s;
}

inline PwArgs pw_args(int n, int n0, int K, int C, const float* q, const float* s, const int* idx, const float* cen, const float* nbr, const float* wp, float radius,
                      int bn_mode, const float* gamma, const float* beta, const float* mean, const float* invstd, int act, int red, const int* padding_num)
{
    PwArgs a;
    a.n = n; a.n0 = n0; a.K = K; a.C = C; a.L = C / 4; a.tpb = PW_BLOCK / a.L;
    a.q = q; a.s = s; a.idx = idx; a.cen = cen; a.nbr = nbr; a.wp = wp; a.inv_radius = 1.0f / radius;
    a.bn_mode = bn_mode; a.act = act; a.red = red; a.gamma = gamma; a.beta = beta; a.mean = mean; a.invstd = invstd; a.padding_num = padding_num;
    return a;
}
inline unsigned pw_grid(int rows, int tpb, int cap) { return cbl_grid_for(((long long)rows + tpb - 1) / tpb, 1, cap); }

}  // namespace

CBL_EXPORT size_t cbl_pointwise_mlp_workspace_bytes(int n, int n0, int K, int C_out)
{
    if (pw_check(n, n0, K, C_out, 1.f, 0, 0, 0) != CBL_OK) return 0;
    return pw_space(n, C_out).total + 256;
}

CBL_EXPORT int cbl_pointwise_mlp_forward(int n, int n0, int K, int C_out, const float* query_points, const float* support_points, const int* neighbors_indices,
                                         const float* center_term, const float* neighbor_term, const float* w_pos, float radius,
                                         int bn_mode, const float* gamma, const float* beta, float eps, float momentum, float* moving_mean, float* moving_var,
                                         int activation, int reduction, const int* padding_num, float* save_mean, float* save_invstd, float* out,
                                         void* workspace, size_t workspace_bytes, void* stream)
{
    const int rc = pw_check(n, n0, K, C_out, radius, bn_mode, activation, reduction);
    if (rc) return rc;
    if (n == 0) return CBL_OK;
    if (!query_points || !support_points || !neighbors_indices || !neighbor_term || !out || (reduction == PW_MEAN && !padding_num)) return CBL_ERR_BAD_ARG;
    if (bn_mode != PW_BN_NONE && (!save_mean || !save_invstd || !(eps > 0.f))) return CBL_ERR_BAD_ARG;
    if (bn_mode == PW_BN_MOVING && (!moving_mean || !moving_var)) return CBL_ERR_BAD_ARG;
    if (bn_mode == PW_BN_BATCH && (!workspace || !cbl_host_aligned16(workspace))) return CBL_ERR_BAD_ARG;
    if (bn_mode == PW_BN_BATCH && workspace_bytes < cbl_pointwise_mlp_workspace_bytes(n, n0, K, C_out)) return CBL_ERR_WORKSPACE;
    if (!cbl_host_aligned16(center_term) || !cbl_host_aligned16(neighbor_term) || !cbl_host_aligned16(w_pos) || !cbl_host_aligned16(out) ||
        !cbl_host_aligned16(gamma) || !cbl_host_aligned16(beta) || !cbl_host_aligned16(save_mean) || !cbl_host_aligned16(save_invstd)) return CBL_ERR_UNSUPPORTED;
    hipStream_t st = cbl_stream(stream);
    const PwArgs a = pw_args(n, n0, K, C_out, query_points, support_points, neighbors_indices, center_term, neighbor_term, w_pos, radius, bn_mode, gamma, beta,
                             save_mean, save_invstd, activation, reduction, padding_num);
    if (bn_mode == PW_BN_BATCH) {
        double* partial = reinterpret_cast<double*>(workspace);
        const unsigned g = pw_grid(n, a.tpb, PW_MAX_BLOCKS);
        hipLaunchKernelGGL(pw_stats_kernel, dim3(g), dim3(PW_BLOCK), 0, st, a, partial);
        hipLaunchKernelGGL(pw_finalize_kernel, dim3(cbl_div_up(C_out, PW_FIN_CH)), dim3(256), 0, st, (int)PW_FIN_STATS, C_out, (int)g, (const double*)partial,
                           (double)n * (double)K, eps, momentum, moving_mean, moving_var, save_mean, save_invstd, (float*)nullptr);
    } else if (bn_mode == PW_BN_MOVING) {
        hipLaunchKernelGGL(pw_moving_kernel, dim3(cbl_div_up(C_out, 256)), dim3(256), 0, st, C_out, (const float*)moving_mean, (const float*)moving_var, eps,
                           save_mean, save_invstd);
    }
    hipLaunchKernelGGL(pw_forward_kernel, dim3(pw_grid(n, a.tpb, 8192)), dim3(PW_BLOCK), 0, st, a, out);
    return cbl_status();
}

CBL_EXPORT int cbl_pointwise_mlp_backward_csr(int n, int n0, int K, int C_out, const float* query_points, const float* support_points, const int* neighbors_indices,
                                              const float* center_term, const float* neighbor_term, const float* w_pos, float radius,
                                              int bn_mode, const float* gamma, const float* beta, const float* save_mean, const float* save_invstd,
                                              int activation, int reduction, const int* padding_num, const float* out, const float* grad_out,
                                              const int* order_dst, const int* inv_start, const int* inv_src,
                                              float* grad_center, float* grad_neighbor, float* grad_w_pos, float* grad_gamma, float* grad_beta,
                                              void* workspace, size_t workspace_bytes, void* stream)
{
    const int rc = pw_check(n, n0, K, C_out, radius, bn_mode, activation, reduction);
    if (rc) return rc;
    if (!grad_center && !grad_neighbor && !grad_w_pos && !grad_gamma && !grad_beta) return CBL_OK;
    if (n > 0 && (!query_points || !support_points || !neighbors_indices || !neighbor_term || !grad_out || (reduction == PW_MEAN && !padding_num) ||
                  (reduction == PW_MAX && !out))) return CBL_ERR_BAD_ARG;
    if (bn_mode != PW_BN_NONE && (!save_mean || !save_invstd)) return CBL_ERR_BAD_ARG;
    if (grad_neighbor && n0 > 0 && (!inv_start || !inv_src || !support_points || !neighbor_term)) return CBL_ERR_BAD_ARG;
    if (grad_w_pos && !w_pos) return CBL_ERR_BAD_ARG;
    if (!workspace || !cbl_host_aligned16(workspace)) return CBL_ERR_BAD_ARG;
    if (workspace_bytes < cbl_pointwise_mlp_workspace_bytes(n, n0, K, C_out)) return CBL_ERR_WORKSPACE;
    if (!cbl_host_aligned16(center_term) || !cbl_host_aligned16(neighbor_term) || !cbl_host_aligned16(w_pos) || !cbl_host_aligned16(out) ||
        !cbl_host_aligned16(grad_out) || !cbl_host_aligned16(gamma) || !cbl_host_aligned16(beta) || !cbl_host_aligned16(save_mean) ||
        !cbl_host_aligned16(save_invstd) || !cbl_host_aligned16(grad_center) || !cbl_host_aligned16(grad_neighbor)) return CBL_ERR_UNSUPPORTED;
    hipStream_t st = cbl_stream(stream);
    const PwSpace sp = pw_space(n, C_out);
    char* base = reinterpret_cast<char*>(workspace);
    double* partial = reinterpret_cast<double*>(base + sp.partial);
    float* coef = reinterpret_cast<float*>(base + sp.coef);
    const PwArgs a = pw_args(n, n0, K, C_out, query_points, support_points, neighbors_indices, center_term, neighbor_term, w_pos, radius, bn_mode, gamma, beta,
                             save_mean, save_invstd, activation, reduction, padding_num);
    PwBwd w;
    w.go = grad_out; w.out = out; w.coef = coef; w.inv_nn = reinterpret_cast<float*>(base + sp.inv_nn); w.ties = reinterpret_cast<float*>(base + sp.ties);
    const double N = (double)n * (double)K;
    if (n == 0) {                                                    // no pair: every sum is empty
        if (grad_neighbor && n0 > 0) (void)hipMemsetAsync(grad_neighbor, 0, sizeof(float) * (size_t)n0 * C_out, st);
        if (grad_w_pos) (void)hipMemsetAsync(grad_w_pos, 0, sizeof(float) * 3 * (size_t)C_out, st);
        if (grad_gamma) (void)hipMemsetAsync(grad_gamma, 0, sizeof(float) * (size_t)C_out, st);
        if (grad_beta) (void)hipMemsetAsync(grad_beta, 0, sizeof(float) * (size_t)C_out, st);
        return cbl_status();
    }
    hipLaunchKernelGGL(pw_inv_count_kernel, dim3(cbl_grid_for(n, 256)), dim3(256), 0, st, n, K, neighbors_indices, padding_num, reduction,
                       reinterpret_cast<float*>(base + sp.inv_nn));
    const unsigned gs = pw_grid(n, a.tpb, PW_MAX_BLOCKS);
    const int sums = bn_mode != PW_BN_NONE ? 1 : 0;
    if (sums || reduction == PW_MAX)
        hipLaunchKernelGGL(pw_bwd_sums_kernel, dim3(gs), dim3(PW_BLOCK), 0, st, a, w, sums, partial);
    if (sums)
        hipLaunchKernelGGL(pw_finalize_kernel, dim3(cbl_div_up(C_out, PW_FIN_CH)), dim3(256), 0, st, (int)PW_FIN_BN_BWD, C_out, (int)gs, (const double*)partial, N, 0.f, 0.f,
                           (float*)nullptr, (float*)nullptr, grad_gamma, grad_beta, coef);
    if (grad_center || grad_w_pos) {
        hipLaunchKernelGGL(pw_bwd_query_kernel, dim3(gs), dim3(PW_BLOCK), 0, st, a, w, grad_center, grad_w_pos ? 1 : 0, partial);
        if (grad_w_pos)
            hipLaunchKernelGGL(pw_finalize_kernel, dim3(cbl_div_up(C_out, PW_FIN_CH)), dim3(256), 0, st, (int)PW_FIN_WPOS, C_out, (int)gs, (const double*)partial, N, 0.f, 0.f,
                               (float*)nullptr, (float*)nullptr, grad_w_pos, (float*)nullptr, (float*)nullptr);
    }
    if (grad_neighbor && n0 > 0)
        hipLaunchKernelGGL(pw_bwd_target_kernel, dim3(pw_grid(n0, a.tpb, 8192)), dim3(PW_BLOCK), 0, st, a, w, cbl_fastdiv_make((unsigned)K), order_dst, inv_start,
                           inv_src, grad_neighbor);
    return cbl_status();
}

// a15  The batch norm + activation that follows every local aggregation of the ConvNet (tensorflow/models/local_aggregation_operators.py:232-249, :304-311,
//      :482-500, :730-745: batch_norm(..., scope='pool_bn') = tf.layers.batch_normalization, then relu / leaky_relu(0.2)): for x (rows, C)
//     out = act(bn(x))
// forward and backward, any 1 <= C <= 4096 and any number of rows.  The batch norm's conventions, its argument checks and the kernels that
// are the unary entries' too come from tf_bn.h; what is here is the statistics scheme and the element passes of rows that are an INPUT, not a product.
//   threads  : a thread owns one group of four columns (one 16-byte load a row) and every nrl-th row of its workgroup's rows: a workgroup covers a slab of
//              w <= 64 column groups with nrl = 256 / w row lanes (thread = row lane * w + column group), so a narrow C still fills the workgroup: C = 72 is
//              18 groups x 14 row lanes.  A thread fetches 8 rows at a time (eight independent 16-byte loads in flight).  Widths that are no multiple of 4
//              and bases that are not 16-byte aligned take scalar loads and stores (vec == 0).
//   bn_mode 1: statistics are CENTRED at every level — a thread takes its rows relative to its first row (the pivot), 8 rows give their own mean and sum
//              of squares about it, merged into the thread's running (count, mean, M2) by Chan's update: every rounding is of the size of the column's
//              spread, not of its mean.  The workgroup's row lanes (pivot + mean in fp64) are combined in fp64 in lane order (mean first, then M2 about
//              it); the workgroups' (mean as two floats, M2) partials are combined in fp64 in chunk order.  There is no sum of x^2 anywhere.
//   launches : rows <= PB_SMALL_ROWS: ONE launch per call — a workgroup owns a slab of <= 8 column groups over ALL rows (32 row lanes), takes the statistics
//              (forward) or the two column sums (backward), finishes them in LDS and walks its rows again (they come from the L2): few rows at a wide C
//              (a coarse layer of a small scene) are a matter of launches, not of bytes.  More rows: grids of (row chunks, slabs); forward =
//              statistics, finalize, element pass (12 rows C bytes), backward = sums (reads grad_out, out, x), finalize, element pass (reads the three, writes
//              grad_x): 28 rows C bytes.  The rule depends on rows alone.
// No float atomics; every output is stored once in a fixed summation order (the grids depend on the shapes alone); no allocation or synchronisation.
#include "tf_bn.h"                                                // and through it pair_tile.h: pair_act / pair_dact, pair_f32x4, pair_up256

namespace {

constexpr int PB_BLOCK = 256, PB_MAX_C = 4096;
constexpr int PB_SLAB = 64, PB_SMALL_SLAB = 8;                      // the most column groups of a workgroup's slab: chunked launches, the single launch
constexpr int PB_BATCH = 8;                                         // rows a thread fetches at a time
constexpr int PB_MAX_CHUNKS = 512;                                  // grid cap (blockIdx.x) of the chunked kernels: past it a chunk holds more rows
constexpr long long PB_SMALL_ROWS = 512;                            // at most this many rows: the single launch (measured: DESIGN.md 6.15)

struct PbGeom { int ncg, w, nrl, slabs; };                          // column groups; of a slab; row lanes; slabs
inline PbGeom pb_geom(int C, int max_w)
{
    PbGeom g;
    g.ncg = (C + 3) / 4;
    g.slabs = (g.ncg + max_w - 1) / max_w;
    g.w = (g.ncg + g.slabs - 1) / g.slabs;
    g.nrl = PB_BLOCK / g.w;
    return g;
}

// this thread's place: column group cg of the slab blockIdx.y, row lane rl (active: rl < nrl and the group exists)
struct PbThread { int rl, c, nv; bool on; };
__device__ __forceinline__ PbThread pb_thread(int C, int ncg, int w, int nrl)
{
    PbThread t;
    t.rl = threadIdx.x / w;
    const int cg = (int)blockIdx.y * w + (threadIdx.x - t.rl * w);
    t.c = 4 * cg;
    t.nv = C - t.c < 4 ? C - t.c : 4;
    t.on = t.rl < nrl && cg < ncg;
    return t;
}

// rows r0 + rl, + nrl, ... < r1 of this thread's four columns, PB_BATCH at a time: f(batch, count) with the rows past r1 as zeros
template <class F>
__device__ __forceinline__ void pb_rows(const float* __restrict__ x, int C, bool vec, const PbThread& t, int nrl, long long r0, long long r1, F f)
{
    for (long long r = r0 + t.rl; r < r1; r += (long long)PB_BATCH * nrl) {
        pair_f32x4 v[PB_BATCH];
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < PB_BATCH; j++) {
            const long long rr = r + (long long)j * nrl;
            v[j] = pair_f32x4{0.f, 0.f, 0.f, 0.f};
            if (rr < r1) { v[j] = tfbn_ld4(x + (size_t)rr * C + t.c, vec, t.nv); cnt = j + 1; }
        }
        f(v, cnt);
    }
}

// the statistics of this thread's rows, centred: n, and about the pivot k[4] (the thread's first row) mean[4] and m2[4] (m2 = the sum of squares about
// k + mean).  Every value is taken relative to the pivot before anything is summed: what is rounded is of the size of the column's spread, not of its mean
__device__ __forceinline__ void pb_thread_stats(const float* __restrict__ x, int C, bool vec, const PbThread& t, int nrl, long long r0, long long r1, float& n,
                                                pair_f32x4& k, pair_f32x4& mean, pair_f32x4& m2)
{
    n = 0.f;
    k = pair_f32x4{0.f, 0.f, 0.f, 0.f};
    mean = pair_f32x4{0.f, 0.f, 0.f, 0.f};
    m2 = pair_f32x4{0.f, 0.f, 0.f, 0.f};
    if (!t.on) return;
    pb_rows(x, C, vec, t, nrl, r0, r1, [&](const pair_f32x4 (&u)[PB_BATCH], int cnt) {
        if (n == 0.f) k = u[0];
        pair_f32x4 v[PB_BATCH];
        pair_f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < PB_BATCH; j++) {                         // (rows past the count stay zeros)
            v[j] = pair_f32x4{0.f, 0.f, 0.f, 0.f};
            if (j < cnt) { v[j] = u[j] - k; s = s + v[j]; }
        }
        const float nb = (float)cnt, inv = 1.f / nb;
        pair_f32x4 lm, lq = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; q++) lm[q] = s[q] * inv;
#pragma unroll
        for (int j = 0; j < PB_BATCH; j++)
            if (j < cnt) { const pair_f32x4 d = v[j] - lm; lq = lq + d * d; }
        // Chan: (n, mean, m2) <- (n, mean, m2) + (nb, lm, lq)
        const float tot = n + nb, fb = nb / tot, fab = n * fb;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const float d = lm[q] - mean[q];
            mean[q] = mean[q] + d * fb;
            m2[q] = (m2[q] + lq[q]) + (d * d) * fab;
        }
        n = tot;
    });
}

// LDS of a workgroup: the row lanes' statistics (forward) or column sums (backward), then the slab's finished per-column values
struct PbShared {
    union {                                                         // a kernel is forward or backward: the two share the bytes (16 KB)
        struct { float n[PB_BLOCK], k[PB_BLOCK][4], a[PB_BLOCK][4], b[PB_BLOCK][4]; };   // forward: count, pivot, mean about it, m2
        struct { double s1[PB_BLOCK][4], s2[PB_BLOCK][4]; };        // backward: sum dz, sum dz * xhat
    };
    float col[4][4 * PB_SLAB];                                      // per column of the slab: forward mean, invstd; backward sum dz / N, sum dz xhat / N
};

// the row lanes' (n, pivot + mean, m2) of column j of the slab (thread j < 4 w), combined in fp64 in lane order: the mean first, about the first lane's
// pivot, then M2 about it.  -> N
__device__ __forceinline__ double pb_combine_stats(const PbShared& S, int w, int nrl, int j, double& mean, double& m2)
{
    const int cg = j >> 2, q = j & 3;
    const double k0 = (double)S.k[cg][q];                            // (lane 0 of a workgroup with any row has one)
    double sum = 0.0, N = 0.0;
    for (int l = 0; l < nrl; l++) { const int t = l * w + cg; sum += (double)S.n[t] * (((double)S.k[t][q] - k0) + (double)S.a[t][q]); N += (double)S.n[t]; }
    const double rel = N > 0.0 ? sum / N : 0.0;
    mean = k0 + rel;
    m2 = 0.0;
    for (int l = 0; l < nrl; l++) {
        const int t = l * w + cg;
        const double d = (((double)S.k[t][q] - k0) + (double)S.a[t][q]) - rel;
        m2 += (double)S.b[t][q] + (double)S.n[t] * d * d;
    }
    return N;
}

struct PbForward {
    long long rows, chunk_rows;
    int C, ncg, w, nrl, vec, bn_mode, act;
    float eps, momentum;
    const float *x, *gamma, *beta;
    float *moving_mean, *moving_var, *save_mean, *save_invstd, *out;
    float* part;                                                    // (chunks, C, 3) per column: a chunk's mean as hi + lo (its fp64 value's two halves) and M2
};

// out = act(bn(x)) over rows [r0, r1) of this thread's columns, the statistics read from mean / invstd (indexed by column)
__device__ __forceinline__ void pb_normalize_rows(const PbForward& a, const PbThread& t, long long r0, long long r1, pair_f32x4 mean, pair_f32x4 invstd)
{
    if (!t.on) return;
    pair_f32x4 g = {1.f, 1.f, 1.f, 1.f}, b = {0.f, 0.f, 0.f, 0.f};
    if (a.bn_mode)
#pragma unroll
        for (int q = 0; q < 4; q++) if (q < t.nv) { g[q] = a.gamma[t.c + q]; b[q] = a.beta[t.c + q]; }
    long long r = r0 + t.rl;
    pb_rows(a.x, a.C, a.vec != 0, t, a.nrl, r0, r1, [&](const pair_f32x4 (&v)[PB_BATCH], int cnt) {
#pragma unroll
        for (int j = 0; j < PB_BATCH; j++) {
            if (j >= cnt) continue;
            pair_f32x4 o;
#pragma unroll
            for (int q = 0; q < 4; q++) o[q] = pair_act(a.act, a.bn_mode ? tfbn_xhat(v[j][q], mean[q], invstd[q]) * g[q] + b[q] : v[j][q]);
            tfbn_st4(a.out + (size_t)(r + (long long)j * a.nrl) * a.C + t.c, o, a.vec != 0, t.nv);
        }
        r += (long long)PB_BATCH * a.nrl;
    });
}


// the single launch: grid (1, slabs); every bn_mode
__global__ __launch_bounds__(PB_BLOCK) void pb_forward_small_kernel(PbForward a)
{
    __shared__ PbShared S;
    const PbThread t = pb_thread(a.C, a.ncg, a.w, a.nrl);
    const int j = threadIdx.x, c = 4 * (int)blockIdx.y * a.w + j;    // thread j < 4 w: column j of the slab
    const bool colthread = j < 4 * a.w && c < a.C;
    if (a.bn_mode == 1) {
        float n;
        pair_f32x4 k, mean, m2;
        pb_thread_stats(a.x, a.C, a.vec != 0, t, a.nrl, 0, a.rows, n, k, mean, m2);
        S.n[threadIdx.x] = n;
#pragma unroll
        for (int q = 0; q < 4; q++) { S.k[threadIdx.x][q] = k[q]; S.a[threadIdx.x][q] = mean[q]; S.b[threadIdx.x][q] = m2[q]; }
        __syncthreads();
        if (colthread) {
            double dm, dq;
            const double N = pb_combine_stats(S, a.w, a.nrl, j, dm, dq);
            tfbn_finish_stats(c, N, dm, dq, a.eps, a.momentum, a.moving_mean, a.moving_var, a.save_mean, a.save_invstd, S.col[0][j], S.col[1][j]);
        }
    } else if (a.bn_mode == 2 && colthread) {
        a.save_mean[c] = S.col[0][j] = a.moving_mean[c];
        a.save_invstd[c] = S.col[1][j] = tfbn_moving_invstd(a.moving_var[c], a.eps);
    }
    __syncthreads();
    pair_f32x4 mean = {0.f, 0.f, 0.f, 0.f}, invstd = {1.f, 1.f, 1.f, 1.f};
    if (a.bn_mode && t.on)
#pragma unroll
        for (int q = 0; q < 4; q++) if (q < t.nv) { const int jj = t.c - 4 * (int)blockIdx.y * a.w + q; mean[q] = S.col[0][jj]; invstd[q] = S.col[1][jj]; }
    pb_normalize_rows(a, t, 0, a.rows, mean, invstd);
}

// chunked, bn_mode 1, first pass: grid (chunks, slabs); a chunk's (mean, M2) per column
__global__ __launch_bounds__(PB_BLOCK) void pb_stats_kernel(PbForward a)
{
    __shared__ PbShared S;
    const PbThread t = pb_thread(a.C, a.ncg, a.w, a.nrl);
    const long long r0 = (long long)blockIdx.x * a.chunk_rows, r1 = r0 + a.chunk_rows < a.rows ? r0 + a.chunk_rows : a.rows;
    float n;
    pair_f32x4 k, mean, m2;
    pb_thread_stats(a.x, a.C, a.vec != 0, t, a.nrl, r0, r1, n, k, mean, m2);
    S.n[threadIdx.x] = n;
#pragma unroll
    for (int q = 0; q < 4; q++) { S.k[threadIdx.x][q] = k[q]; S.a[threadIdx.x][q] = mean[q]; S.b[threadIdx.x][q] = m2[q]; }
    __syncthreads();
    const int j = threadIdx.x, c = 4 * (int)blockIdx.y * a.w + j;
    if (j < 4 * a.w && c < a.C) {
        double dm, dq;
        pb_combine_stats(S, a.w, a.nrl, j, dm, dq);
        float* dst = a.part + ((size_t)blockIdx.x * a.C + c) * 3;
        dst[0] = (float)dm;
        dst[1] = (float)(dm - (double)dst[0]);
        dst[2] = (float)dq;
    }
}

// the chunks' (count, mean, M2) -> the batch statistics of every column, in fp64 and chunk order: 32 columns a workgroup, eight shares of the chunks each,
// the shares summed in share order (ul_stats_finalize_kernel's scheme with the chunk's row count in the place of the tile's); the means are summed about
// the first chunk's
__global__ __launch_bounds__(PB_BLOCK) void pb_stats_finalize_kernel(PbForward a, int nchunks)
{
    __shared__ double red[8][32];
    const int cl = threadIdx.x & 31, g = threadIdx.x >> 5, c = blockIdx.x * 32 + cl;
    const bool ok = c < a.C;
    auto count = [&](int k) { const long long left = a.rows - (long long)k * a.chunk_rows; return (double)(left < a.chunk_rows ? left : a.chunk_rows); };
    auto mean_of = [&](int k) { const float* p = a.part + ((size_t)k * a.C + c) * 3; return (double)p[0] + (double)p[1]; };
    const double pivot = ok ? mean_of(0) : 0.0;
    double s = 0.0;
    if (ok)
        for (int k = g; k < nchunks; k += 8) s += count(k) * (mean_of(k) - pivot);
    red[g][cl] = s;
    __syncthreads();
    double rel = 0.0;
    for (int i = 0; i < 8; i++) rel += red[i][cl];
    rel /= (double)a.rows;
    const double mean = pivot + rel;
    __syncthreads();
    double m2 = 0.0;
    if (ok)
        for (int k = g; k < nchunks; k += 8) {
            const double d = (mean_of(k) - pivot) - rel;
            m2 += (double)a.part[((size_t)k * a.C + c) * 3 + 2] + count(k) * d * d;
        }
    red[g][cl] = m2;
    __syncthreads();
    if (g == 0 && ok) {
        double tot = 0.0;
        for (int i = 0; i < 8; i++) tot += red[i][cl];
        float fm, fi;
        tfbn_finish_stats(c, (double)a.rows, mean, tot, a.eps, a.momentum, a.moving_mean, a.moving_var, a.save_mean, a.save_invstd, fm, fi);
    }
}

// chunked, the element pass: grid (chunks, slabs)
__global__ __launch_bounds__(PB_BLOCK) void pb_normalize_kernel(PbForward a)
{
    const PbThread t = pb_thread(a.C, a.ncg, a.w, a.nrl);
    const long long r0 = (long long)blockIdx.x * a.chunk_rows, r1 = r0 + a.chunk_rows < a.rows ? r0 + a.chunk_rows : a.rows;
    pair_f32x4 mean = {0.f, 0.f, 0.f, 0.f}, invstd = {1.f, 1.f, 1.f, 1.f};
    if (a.bn_mode && t.on)
#pragma unroll
        for (int q = 0; q < 4; q++) if (q < t.nv) { mean[q] = a.save_mean[t.c + q]; invstd[q] = a.save_invstd[t.c + q]; }
    pb_normalize_rows(a, t, r0, r1, mean, invstd);
}

struct PbBackward {
    long long rows, chunk_rows;
    int C, ncg, w, nrl, vec, bn_mode, act, want_sums;
    float inv_n;
    const float *x, *gamma, *mean, *invstd, *out, *go, *sums;       // sums (2, C): sum dz, sum dz * xhat (chunked element pass)
    float *gx, *gg, *gb;
    double* part;                                                   // (chunks, C, 2)
};

// rows r0 + rl, + nrl, ... < r1: f(row, dz, x) with dz = grad_out * act'(out) of this thread's four columns.  Three (two, one) independent loads a row
template <class F>
__device__ __forceinline__ void pb_backward_rows(const PbBackward& a, const PbThread& t, bool need_x, long long r0, long long r1, F f)
{
    const bool vec = a.vec != 0;
    for (long long r = r0 + t.rl; r < r1; r += 2ll * a.nrl) {
        const long long rb = r + a.nrl;
        const bool two = rb < r1;
        const size_t oa = (size_t)r * a.C + t.c, ob = (size_t)rb * a.C + t.c;
        const pair_f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        pair_f32x4 ga = tfbn_ld4(a.go + oa, vec, t.nv), gb = two ? tfbn_ld4(a.go + ob, vec, t.nv) : zero;
        const pair_f32x4 ha = a.act ? tfbn_ld4(a.out + oa, vec, t.nv) : zero, hb = (a.act && two) ? tfbn_ld4(a.out + ob, vec, t.nv) : zero;
        const pair_f32x4 xa = need_x ? tfbn_ld4(a.x + oa, vec, t.nv) : zero, xb = (need_x && two) ? tfbn_ld4(a.x + ob, vec, t.nv) : zero;
        if (a.act)
#pragma unroll
            for (int q = 0; q < 4; q++) { ga[q] = ga[q] * pair_dact(a.act, ha[q]); gb[q] = gb[q] * pair_dact(a.act, hb[q]); }
        f(r, ga, xa);
        if (two) f(rb, gb, xb);
    }
}

// this thread's sum dz and sum dz * xhat over its rows of [r0, r1), in fp64
__device__ __forceinline__ void pb_thread_sums(const PbBackward& a, const PbThread& t, long long r0, long long r1, double (&s1)[4], double (&s2)[4])
{
#pragma unroll
    for (int q = 0; q < 4; q++) s1[q] = s2[q] = 0.0;
    if (!t.on) return;
    pair_f32x4 mean = {0.f, 0.f, 0.f, 0.f}, invstd = {1.f, 1.f, 1.f, 1.f};
#pragma unroll
    for (int q = 0; q < 4; q++) if (q < t.nv) { mean[q] = a.mean[t.c + q]; invstd[q] = a.invstd[t.c + q]; }
    pb_backward_rows(a, t, true, r0, r1, [&](long long, const pair_f32x4& dz, const pair_f32x4& x) {
#pragma unroll
        for (int q = 0; q < 4; q++) { s1[q] += (double)dz[q]; s2[q] += (double)(dz[q] * tfbn_xhat(x[q], mean[q], invstd[q])); }
    });
}

// grad_x over rows [r0, r1): s1n, s2n = sum dz / N, sum dz xhat / N of this thread's columns (bn_mode 1)
__device__ __forceinline__ void pb_dx_rows(const PbBackward& a, const PbThread& t, long long r0, long long r1, pair_f32x4 s1n, pair_f32x4 s2n)
{
    if (!t.on) return;
    pair_f32x4 mean = {0.f, 0.f, 0.f, 0.f}, invstd = {1.f, 1.f, 1.f, 1.f}, gi = {1.f, 1.f, 1.f, 1.f};
    if (a.bn_mode)
#pragma unroll
        for (int q = 0; q < 4; q++) if (q < t.nv) { mean[q] = a.mean[t.c + q]; invstd[q] = a.invstd[t.c + q]; gi[q] = a.gamma[t.c + q] * invstd[q]; }
    pb_backward_rows(a, t, a.bn_mode == 1, r0, r1, [&](long long row, const pair_f32x4& dz, const pair_f32x4& x) {
        pair_f32x4 dx;
#pragma unroll
        for (int q = 0; q < 4; q++)
            dx[q] = a.bn_mode == 1 ? gi[q] * ((dz[q] - s1n[q]) - tfbn_xhat(x[q], mean[q], invstd[q]) * s2n[q]) : a.bn_mode == 2 ? gi[q] * dz[q] : dz[q];
        tfbn_st4(a.gx + (size_t)row * a.C + t.c, dx, a.vec != 0, t.nv);
    });
}

// the row lanes' sums of column j of the slab, in lane order
__device__ __forceinline__ void pb_combine_sums(const PbShared& S, int w, int nrl, int j, double& s1, double& s2)
{
    const int cg = j >> 2, q = j & 3;
    s1 = s2 = 0.0;
    for (int l = 0; l < nrl; l++) { s1 += S.s1[l * w + cg][q]; s2 += S.s2[l * w + cg][q]; }
}

// the single launch: grid (1, slabs)
__global__ __launch_bounds__(PB_BLOCK) void pb_backward_small_kernel(PbBackward a)
{
    __shared__ PbShared S;
    const PbThread t = pb_thread(a.C, a.ncg, a.w, a.nrl);
    if (a.want_sums) {
        double s1[4], s2[4];
        pb_thread_sums(a, t, 0, a.rows, s1, s2);
#pragma unroll
        for (int q = 0; q < 4; q++) { S.s1[threadIdx.x][q] = s1[q]; S.s2[threadIdx.x][q] = s2[q]; }
        __syncthreads();
        const int j = threadIdx.x, c = 4 * (int)blockIdx.y * a.w + j;
        if (j < 4 * a.w && c < a.C) {
            double d1, d2;
            pb_combine_sums(S, a.w, a.nrl, j, d1, d2);
            const float f1 = (float)d1, f2 = (float)d2;
            if (a.gb) a.gb[c] = f1;
            if (a.gg) a.gg[c] = f2;
            S.col[2][j] = f1 * a.inv_n;
            S.col[3][j] = f2 * a.inv_n;
        }
        __syncthreads();
    }
    if (!a.gx) return;
    pair_f32x4 s1n = {0.f, 0.f, 0.f, 0.f}, s2n = {0.f, 0.f, 0.f, 0.f};
    if (a.bn_mode == 1 && t.on)
#pragma unroll
        for (int q = 0; q < 4; q++) if (q < t.nv) { const int jj = t.c - 4 * (int)blockIdx.y * a.w + q; s1n[q] = S.col[2][jj]; s2n[q] = S.col[3][jj]; }
    pb_dx_rows(a, t, 0, a.rows, s1n, s2n);
}

// chunked, first pass: grid (chunks, slabs); a chunk's two sums per column
__global__ __launch_bounds__(PB_BLOCK) void pb_sums_kernel(PbBackward a)
{
    __shared__ PbShared S;
    const PbThread t = pb_thread(a.C, a.ncg, a.w, a.nrl);
    const long long r0 = (long long)blockIdx.x * a.chunk_rows, r1 = r0 + a.chunk_rows < a.rows ? r0 + a.chunk_rows : a.rows;
    double s1[4], s2[4];
    pb_thread_sums(a, t, r0, r1, s1, s2);
#pragma unroll
    for (int q = 0; q < 4; q++) { S.s1[threadIdx.x][q] = s1[q]; S.s2[threadIdx.x][q] = s2[q]; }
    __syncthreads();
    const int j = threadIdx.x, c = 4 * (int)blockIdx.y * a.w + j;
    if (j < 4 * a.w && c < a.C) {
        double* dst = a.part + ((size_t)blockIdx.x * a.C + c) * 2;
        pb_combine_sums(S, a.w, a.nrl, j, dst[0], dst[1]);
    }
}
// (the chunks' sums in chunk order — grad_beta, grad_gamma and the two values the element pass reads —: tfbn_sums_finalize_kernel)

// chunked, the element pass: grid (chunks, slabs)
__global__ __launch_bounds__(PB_BLOCK) void pb_dx_kernel(PbBackward a)
{
    const PbThread t = pb_thread(a.C, a.ncg, a.w, a.nrl);
    const long long r0 = (long long)blockIdx.x * a.chunk_rows, r1 = r0 + a.chunk_rows < a.rows ? r0 + a.chunk_rows : a.rows;
    pair_f32x4 s1n = {0.f, 0.f, 0.f, 0.f}, s2n = {0.f, 0.f, 0.f, 0.f};
    if (a.bn_mode == 1 && t.on)
#pragma unroll
        for (int q = 0; q < 4; q++) if (q < t.nv) { s1n[q] = a.sums[t.c + q] * a.inv_n; s2n[q] = a.sums[a.C + t.c + q] * a.inv_n; }
    pb_dx_rows(a, t, r0, r1, s1n, s2n);
}

// ---------------------------------------------------------------- host side
struct PbPlan {
    bool small;
    PbGeom g;
    long long chunk_rows;
    int nchunks;
    size_t off_part, off_sumpart, off_sums, bytes;                  // byte offsets from the (256-byte aligned) workspace base
};
inline PbPlan pb_plan(long long rows, int C)
{
    PbPlan p;
    p.small = rows <= PB_SMALL_ROWS;
    // the chunked geometry (sized whatever the rule says, so that the workspace is one size).  A chunk: at least one fetch of every row lane, and no more
    // chunks than the cap
    const PbGeom g = pb_geom(C, PB_SLAB);
    const long long least = (long long)g.nrl * PB_BATCH;
    long long nchunks = (rows + least - 1) / least;
    if (nchunks > PB_MAX_CHUNKS) nchunks = PB_MAX_CHUNKS;
    if (nchunks < 1) nchunks = 1;
    p.chunk_rows = (rows + nchunks - 1) / nchunks;
    if (p.chunk_rows < 1) p.chunk_rows = 1;
    p.nchunks = (int)((rows + p.chunk_rows - 1) / p.chunk_rows);
    if (p.nchunks < 1) p.nchunks = 1;
    p.g = p.small ? pb_geom(C, PB_SMALL_SLAB) : g;
    size_t o = 0;
    p.off_part = o;    o += pair_up256((size_t)p.nchunks * C * 3 * sizeof(float));
    p.off_sumpart = o; o += pair_up256((size_t)p.nchunks * C * 2 * sizeof(double));
    p.off_sums = o;    o += pair_up256((size_t)C * 2 * sizeof(float));
    p.bytes = o + 256;                                              // the base is rounded up to 256 bytes
    return p;
}

}  // namespace

CBL_EXPORT size_t cbl_pool_bn_workspace_bytes(long long rows, int C)
{
    if (rows < 0 || C < 1 || C > PB_MAX_C) return 0;
    return pb_plan(rows, C).bytes;
}

CBL_EXPORT int cbl_pool_bn_forward(long long rows, int C, const float* x, int bn_mode, const float* gamma, const float* beta, float eps, float momentum,
                                   float* moving_mean, float* moving_var, int activation, float* save_mean, float* save_invstd, float* out, void* workspace,
                                   size_t workspace_bytes, void* stream)
{
    if (rows < 0 || C < 1 || !tfbn_modes_ok(bn_mode, activation)) return CBL_ERR_BAD_ARG;
    if (C > PB_MAX_C) return CBL_ERR_UNSUPPORTED;
    if (rows == 0) return CBL_OK;
    if (!x || !out) return CBL_ERR_BAD_ARG;
    if (const int rc = tfbn_check_forward(bn_mode, gamma, beta, eps, moving_mean, moving_var, save_mean, save_invstd)) return rc;
    const PbPlan p = pb_plan(rows, C);
    if (bn_mode == 1 && (!workspace || workspace_bytes < p.bytes)) return CBL_ERR_WORKSPACE;
    hipStream_t st = cbl_stream(stream);
    PbForward a;
    a.rows = rows; a.chunk_rows = p.chunk_rows; a.C = C; a.ncg = p.g.ncg; a.w = p.g.w; a.nrl = p.g.nrl; a.vec = tfbn_vec(C, x, out);
    a.bn_mode = bn_mode; a.act = activation; a.eps = eps; a.momentum = momentum;
    a.x = x; a.gamma = gamma; a.beta = beta; a.moving_mean = moving_mean; a.moving_var = moving_var; a.save_mean = save_mean; a.save_invstd = save_invstd;
    a.out = out; a.part = bn_mode == 1 ? reinterpret_cast<float*>(tfbn_base(workspace) + p.off_part) : nullptr;
    if (p.small) {
        hipLaunchKernelGGL(pb_forward_small_kernel, dim3(1, p.g.slabs), dim3(PB_BLOCK), 0, st, a);
        return cbl_status();
    }
    const dim3 grid(p.nchunks, p.g.slabs);
    if (bn_mode == 1) {
        hipLaunchKernelGGL(pb_stats_kernel, grid, dim3(PB_BLOCK), 0, st, a);
        hipLaunchKernelGGL(pb_stats_finalize_kernel, dim3(cbl_div_up(C, 32)), dim3(PB_BLOCK), 0, st, a, p.nchunks);
    } else if (bn_mode == 2)
        tfbn_launch_moving_stats(st, C, moving_mean, moving_var, eps, save_mean, save_invstd);
    hipLaunchKernelGGL(pb_normalize_kernel, grid, dim3(PB_BLOCK), 0, st, a);
    return cbl_status();
}

CBL_EXPORT int cbl_pool_bn_backward(long long rows, int C, const float* x, int bn_mode, const float* gamma, const float* save_mean, const float* save_invstd,
                                    int activation, const float* out, const float* grad_out, float* grad_x, float* grad_gamma, float* grad_beta,
                                    void* workspace, size_t workspace_bytes, void* stream)
{
    if (rows < 0 || C < 1 || !tfbn_modes_ok(bn_mode, activation)) return CBL_ERR_BAD_ARG;
    if (C > PB_MAX_C) return CBL_ERR_UNSUPPORTED;
    if (rows == 0) return CBL_OK;
    if (!grad_out || (bn_mode != 0 && !x)) return CBL_ERR_BAD_ARG;
    if (const int rc = tfbn_check_backward(bn_mode, activation, gamma, save_mean, save_invstd, out, grad_gamma, grad_beta)) return rc;
    const PbPlan p = pb_plan(rows, C);
    if (bn_mode != 0 && (!workspace || workspace_bytes < p.bytes)) return CBL_ERR_WORKSPACE;
    hipStream_t st = cbl_stream(stream);
    char* base = bn_mode != 0 ? tfbn_base(workspace) : nullptr;
    PbBackward a;
    a.rows = rows; a.chunk_rows = p.chunk_rows; a.C = C; a.ncg = p.g.ncg; a.w = p.g.w; a.nrl = p.g.nrl; a.vec = tfbn_vec(C, x, out, grad_out, grad_x);
    a.bn_mode = bn_mode; a.act = activation; a.inv_n = (float)(1.0 / (double)rows);
    a.want_sums = bn_mode == 1 ? (grad_x || grad_gamma || grad_beta) : bn_mode == 2 ? (grad_gamma || grad_beta) : 0;
    a.x = x; a.gamma = gamma; a.mean = save_mean; a.invstd = save_invstd; a.out = out; a.go = grad_out;
    a.sums = base ? reinterpret_cast<float*>(base + p.off_sums) : nullptr;
    a.gx = grad_x; a.gg = grad_gamma; a.gb = grad_beta;
    a.part = base ? reinterpret_cast<double*>(base + p.off_sumpart) : nullptr;
    if (!a.want_sums && !grad_x) return CBL_OK;
    if (p.small) {
        hipLaunchKernelGGL(pb_backward_small_kernel, dim3(1, p.g.slabs), dim3(PB_BLOCK), 0, st, a);
        return cbl_status();
    }
    const dim3 grid(p.nchunks, p.g.slabs);
    if (a.want_sums) {
        hipLaunchKernelGGL(pb_sums_kernel, grid, dim3(PB_BLOCK), 0, st, a);
        tfbn_launch_sums_finalize(st, C, p.nchunks, a.part, const_cast<float*>(a.sums), grad_beta, grad_gamma);
    }
    if (grad_x) hipLaunchKernelGGL(pb_dx_kernel, grid, dim3(PB_BLOCK), 0, st, a);
    return cbl_status();
}

// a14: the gradient of ind_max_pool  (tensorflow/models/basic_operators.py:155-172; the shortcut of every strided bottleneck, models/backbone/resnet.py).
// The graph is  x' = concat(x, reduce_min(x, 0)),  out = reduce_max(gather(x', inds), 1),  and TensorFlow's gradient of reduce_max / reduce_min shares the
// incoming gradient EQUALLY among all tied entries.  Ties are the normal case (the pooled features leave a ReLU: exact zeros everywhere), and the shadow row
// hands its share on to the rows that attain the column minimum, again split among ties — a stored arg-max would be wrong on exactly these inputs.
//   shadow[c] = min_s x[s,c]            v[r,j,c] = x[inds[r,j],c]  (an id outside [0, n1): shadow[c])            out[r,c] = max_j v[r,j,c]
//   cnt[r,c]  = #{j : v[r,j,c] == out[r,c]}     w[r,c] = g[r,c] / cnt[r,c]     S[c] = sum_r w[r,c] * #{j shadow : shadow[c] == out[r,c]}     nmin[c] = #{s : x[s,c] == shadow[c]}
//   grad_x[s,c] = sum over the pairs (r,j) with inds[r,j] == s of [x[s,c] == out[r,c]] * w[r,c]   +   [x[s,c] == shadow[c]] * S[c] / nmin[c]
// All comparisons are float equality: out and shadow are elements of x.  (ind_closest_pool's gradient is cbl_grouping_backward_csr_rows over the table of
// its first column: no kernel here.)
//
// Three passes, no float atomics, every output written with plain stores (gather form, as pointwise_mlp.hip B1 / B3):
//   query pass   walks each pooled row's k entries once more in the forward's layout (ind_max_pool_v4_kernel: lane = V channels of one row, L lanes per row,
//                column chunks of at most 256 lanes, ids one batch ahead of the rows), counts the ties, writes w and reduces the rows' shadow shares to
//                per-workgroup partial sums in fp64 (combined by imp_finalize_kernel in workgroup order: the sum does not depend on the schedule)
//   nmin pass    one pass over x, per-workgroup integer counts added by the same finalize step (no zero fill, no atomics at all)
//   target pass  per source row the pairs of its segment of the transposed table of inds, ascending; then the shadow term; EVERY row of grad_x is written
// V = 4: d % 4 == 0 and 16-byte rows (float4 accesses); V = 1: one channel per lane, any d and alignment.
#include "cbl_common.h"

namespace {

constexpr int IMP_BLOCK = 256;
constexpr int IMP_MAX_BLOCKS = 1024;         // workgroups of the query pass = rows of the partial sums (a multiple of the 8 XCDs)
constexpr int IMP_MIN_BLOCKS = 256;          // workgroups of the minimum-tie count = rows of its partial counts
constexpr int IMP_FIN_COLS = 16, IMP_FIN_GROUPS = 16;

template <int V> __device__ __forceinline__ void imp_ld(const float* __restrict__ p, float (&v)[V])
{
    if constexpr (V == 4) { const float4 t = *reinterpret_cast<const float4*>(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    else v[0] = *p;
}
template <int V> __device__ __forceinline__ void imp_st(float* __restrict__ p, const float (&v)[V])
{
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}
__device__ __forceinline__ float imp_unkey(unsigned key) { return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key); }   // column_min_kernel's keys

// lane = V consecutive channels (columns V * (c_0 + cl) ..) of one row; DV = d / V columns of that width, this launch takes L of them from c_0
struct ImpLane { int ts, cl, tpb, col; bool live; };
template <int V> __device__ __forceinline__ ImpLane imp_lane(int c_0, int L)
{
    ImpLane t;
    t.tpb = IMP_BLOCK / L;
    t.ts = threadIdx.x / L; t.cl = threadIdx.x - t.ts * L;
    t.live = t.ts < t.tpb;
    t.col = V * (c_0 + t.cl);
    return t;
}

// query pass.  partial: (gridDim.x, d) fp64, row b = workgroup b's sum of w * (number of the row's shadow entries that attain its maximum)
template <int V, int U>
__global__ __launch_bounds__(IMP_BLOCK) void imp_bwd_query_kernel(unsigned n2, int n1, int k, int d, int c_0, int L, const float* __restrict__ x,
                                                                  const int* __restrict__ inds, const unsigned* __restrict__ keymin, const float* __restrict__ out,
                                                                  const float* __restrict__ go, float* __restrict__ w, double* __restrict__ partial)
{
    __shared__ double red[IMP_BLOCK][V];
    const ImpLane t = imp_lane<V>(c_0, L);
    double acc[V];
#pragma unroll
    for (int j = 0; j < V; j++) acc[j] = 0.0;
    if (t.live) {
        float sh[V];
#pragma unroll
        for (int j = 0; j < V; j++) sh[j] = imp_unkey(keymin[t.col + j]);
        const unsigned ntrips = (n2 + t.tpb - 1) / t.tpb;
        const unsigned vend = 8 * cbl_xcd_per(ntrips);
        for (unsigned v = blockIdx.x; v < vend; v += gridDim.x) {
            const unsigned r = cbl_xcd_slot(v, ntrips) * t.tpb + t.ts;
            if (r >= n2) continue;
            const int* __restrict__ row = inds + (size_t)r * k;
            float m[V], g[V], cnt[V], nsh[V];
            imp_ld<V>(out + (size_t)r * d + t.col, m);
            imp_ld<V>(go + (size_t)r * d + t.col, g);
#pragma unroll
            for (int j = 0; j < V; j++) cnt[j] = nsh[j] = 0.f;
            int idn[U];
#pragma unroll
            for (int u = 0; u < U; u++) idn[u] = row[min(u, k - 1)];
            for (int k0 = 0; k0 < k; k0 += U) {
                int id[U]; float xr[U][V];
#pragma unroll
                for (int u = 0; u < U; u++) id[u] = idn[u];
#pragma unroll
                for (int u = 0; u < U; u++) idn[u] = row[min(k0 + U + u, k - 1)];        // clamped, unconditional; entries past the row are not counted below
#pragma unroll
                for (int u = 0; u < U; u++) { const bool real = id[u] >= 0 && id[u] < n1; imp_ld<V>(x + (size_t)(real ? id[u] : 0) * d + t.col, xr[u]); }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const bool in = k0 + u < k, real = id[u] >= 0 && id[u] < n1;
#pragma unroll
                    for (int j = 0; j < V; j++) {
                        const bool hit = in && (real ? xr[u][j] : sh[j]) == m[j];
                        cnt[j] += hit ? 1.f : 0.f;
                        nsh[j] += (hit && !real) ? 1.f : 0.f;
                    }
                }
            }
            float wr[V];
#pragma unroll
            for (int j = 0; j < V; j++) {
                wr[j] = cnt[j] > 0.f ? g[j] / cnt[j] : 0.f;               // cnt >= 1 for finite inputs: out is one of the row's values
                acc[j] += (double)wr[j] * (double)nsh[j];
            }
            imp_st<V>(w + (size_t)r * d + t.col, wr);
        }
    }
#pragma unroll
    for (int j = 0; j < V; j++) red[threadIdx.x][j] = acc[j];
    __syncthreads();
    if ((int)threadIdx.x < L) {                                           // row slot 0 of every column: the slots in ascending order
#pragma unroll
        for (int j = 0; j < V; j++) {
            double s = 0.0;
            for (int q = 0; q < t.tpb; q++) s += red[q * L + threadIdx.x][j];
            partial[(size_t)blockIdx.x * d + t.col + j] = s;
        }
    }
}

// nmin_partial[b, c] = #{rows of workgroup b with x[s,c] == shadow[c]}: written by every workgroup (no zero fill, no atomics), summed by imp_finalize_kernel
template <int V>
__global__ __launch_bounds__(IMP_BLOCK) void imp_min_ties_kernel(unsigned n1, int d, int c_0, int L, const float* __restrict__ x, const unsigned* __restrict__ keymin,
                                                                 int* __restrict__ nmin_partial)
{
    __shared__ int red[IMP_BLOCK][V];
    const ImpLane t = imp_lane<V>(c_0, L);
    int cnt[V];
#pragma unroll
    for (int j = 0; j < V; j++) cnt[j] = 0;
    if (t.live) {
        float sh[V];
#pragma unroll
        for (int j = 0; j < V; j++) sh[j] = imp_unkey(keymin[t.col + j]);
        for (unsigned r = blockIdx.x * t.tpb + t.ts; r < n1; r += gridDim.x * t.tpb) {
            float xv[V];
            imp_ld<V>(x + (size_t)r * d + t.col, xv);
#pragma unroll
            for (int j = 0; j < V; j++) cnt[j] += xv[j] == sh[j] ? 1 : 0;
        }
    }
#pragma unroll
    for (int j = 0; j < V; j++) red[threadIdx.x][j] = cnt[j];
    __syncthreads();
    if ((int)threadIdx.x < L) {
#pragma unroll
        for (int j = 0; j < V; j++) {
            int s = 0;
            for (int q = 0; q < t.tpb; q++) s += red[q * L + threadIdx.x][j];
            nmin_partial[(size_t)blockIdx.x * d + t.col + j] = s;
        }
    }
}

// share[c] = (sum over the workgroups b, ascending within each of IMP_FIN_GROUPS interleaved groups, then over the groups, of partial[b, c]) / nmin[c]
__global__ __launch_bounds__(IMP_FIN_COLS * IMP_FIN_GROUPS) void imp_finalize_kernel(int d, int nblocks, const double* __restrict__ partial, int nmin_blocks,
                                                                                      const int* __restrict__ nmin_partial, float* __restrict__ share)
{
    __shared__ double part[IMP_FIN_GROUPS][IMP_FIN_COLS];
    __shared__ int npart[IMP_FIN_GROUPS][IMP_FIN_COLS];
    const int el = threadIdx.x % IMP_FIN_COLS, grp = threadIdx.x / IMP_FIN_COLS;
    const int c = blockIdx.x * IMP_FIN_COLS + el;
    double acc = 0.0;
    int na = 0;
    if (c < d) {
        for (int b = grp; b < nblocks; b += IMP_FIN_GROUPS) acc += partial[(size_t)b * d + c];
        for (int b = grp; b < nmin_blocks; b += IMP_FIN_GROUPS) na += nmin_partial[(size_t)b * d + c];
    }
    part[grp][el] = acc; npart[grp][el] = na;
    __syncthreads();
    if (grp == 0 && c < d) {
        double s = 0.0;
        int nm = 0;
#pragma unroll
        for (int q = 0; q < IMP_FIN_GROUPS; q++) { s += part[q][el]; nm += npart[q][el]; }
        share[c] = nm > 0 ? (float)(s / (double)nm) : 0.f;
    }
}

__global__ __launch_bounds__(IMP_BLOCK) void imp_zero_kernel(size_t n, float* __restrict__ p)
{
    for (size_t i = (size_t)blockIdx.x * IMP_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * IMP_BLOCK) p[i] = 0.f;
}

// target pass: grad_x[s, :] of the source row s = order[tr] (tr without an order) from the pairs p = r * k + j of segment tr, ascending, UB of them in flight
template <int V, int UB>
__global__ __launch_bounds__(IMP_BLOCK) void imp_bwd_target_kernel(unsigned n1, int d, int c_0, int L, CblFastDiv dvK, const float* __restrict__ x,
                                                                   const unsigned* __restrict__ keymin, const float* __restrict__ out, const float* __restrict__ w,
                                                                   const float* __restrict__ share, const int* __restrict__ order, const int* __restrict__ inv_start,
                                                                   const int* __restrict__ inv_src, float* __restrict__ grad_x)
{
    const ImpLane t = imp_lane<V>(c_0, L);
    if (!t.live) return;
    float sh[V], shr[V];
#pragma unroll
    for (int j = 0; j < V; j++) sh[j] = imp_unkey(keymin[t.col + j]);
    imp_ld<V>(share + t.col, shr);
    const unsigned ntrips = (n1 + t.tpb - 1) / t.tpb;
    const unsigned vend = 8 * cbl_xcd_per(ntrips);
    for (unsigned v = blockIdx.x; v < vend; v += gridDim.x) {
        const unsigned tr = cbl_xcd_slot(v, ntrips) * t.tpb + t.ts;
        if (tr >= n1) continue;
        const int s = order ? order[tr] : (int)tr;
        const int e0 = inv_start[tr], e1 = inv_start[tr + 1];
        float xs[V], acc[V];
        imp_ld<V>(x + (size_t)s * d + t.col, xs);
#pragma unroll
        for (int j = 0; j < V; j++) acc[j] = 0.f;
        if (e1 > e0) {
            int pn[UB];
#pragma unroll
            for (int u = 0; u < UB; u++) pn[u] = inv_src[min(e0 + u, e1 - 1)];
            for (int e = e0; e < e1; e += UB) {
                int r[UB]; float o[UB][V], wv[UB][V];
#pragma unroll
                for (int u = 0; u < UB; u++) r[u] = (int)cbl_fastdiv((unsigned)pn[u], dvK);
#pragma unroll
                for (int u = 0; u < UB; u++) pn[u] = inv_src[min(e + UB + u, e1 - 1)];
#pragma unroll
                for (int u = 0; u < UB; u++) { imp_ld<V>(out + (size_t)r[u] * d + t.col, o[u]); imp_ld<V>(w + (size_t)r[u] * d + t.col, wv[u]); }
#pragma unroll
                for (int u = 0; u < UB; u++)
#pragma unroll
                    for (int j = 0; j < V; j++) acc[j] += (e + u < e1 && xs[j] == o[u][j]) ? wv[u][j] : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < V; j++) acc[j] += xs[j] == sh[j] ? shr[j] : 0.f;
        imp_st<V>(grad_x + (size_t)s * d + t.col, acc);
    }
}

// ---------------------------------------------------------------- host side
inline size_t imp_up(size_t b) { return (b + 255) & ~(size_t)255; }
struct ImpSpace { size_t w, partial, share, nmin, total; };
inline ImpSpace imp_space(int n2, int d)
{
    ImpSpace s;
    s.w = 0;
    s.partial = imp_up(sizeof(float) * (size_t)n2 * d);
    s.share = s.partial + imp_up(sizeof(double) * (size_t)IMP_MAX_BLOCKS * d);
    s.nmin = s.share + imp_up(sizeof(float) * (size_t)d);
    s.total = s.nmin + imp_up(sizeof(int) * (size_t)IMP_MIN_BLOCKS * d);
    return s;
}
inline int imp_check(int n1, int n2, int k, int d)
{
    if (n1 <= 0 || n2 < 0 || k <= 0 || d <= 0) return CBL_ERR_BAD_ARG;
    if ((long long)n2 * k > 2147483647ll) return CBL_ERR_UNSUPPORTED;    // a pair id is an int of the transposed table
    return CBL_OK;
}

}  // namespace

CBL_EXPORT size_t cbl_ind_max_pool_backward_workspace_bytes(int n1, int n2, int k, int d)
{
    if (imp_check(n1, n2, k, d) != CBL_OK) return 0;
    return imp_space(n2, d).total;
}

CBL_EXPORT int cbl_ind_max_pool_backward_csr(int n1, int n2, int k, int d, const float* x, const int* inds, const unsigned* keymin_d, const float* out,
                                             const float* grad_out, const int* order, const int* inv_start, const int* inv_src, float* grad_x, void* ws,
                                             size_t ws_bytes, void* stream)
{
    const int rc = imp_check(n1, n2, k, d);
    if (rc) return rc;
    if (!grad_x) return CBL_ERR_BAD_ARG;
    hipStream_t st = cbl_stream(stream);
    if (n2 == 0) {                                                       // no pooled row: no pair, no shadow share
        hipLaunchKernelGGL(imp_zero_kernel, dim3(cbl_grid_for((long long)n1 * d, IMP_BLOCK)), dim3(IMP_BLOCK), 0, st, (size_t)n1 * d, grad_x);
        return cbl_status();
    }
    if (!x || !inds || !keymin_d || !out || !grad_out || !inv_start || !inv_src) return CBL_ERR_BAD_ARG;
    if (!ws || !cbl_host_aligned16(ws)) return CBL_ERR_BAD_ARG;
    if (ws_bytes < cbl_ind_max_pool_backward_workspace_bytes(n1, n2, k, d)) return CBL_ERR_WORKSPACE;
    const ImpSpace sp = imp_space(n2, d);
    char* base = reinterpret_cast<char*>(ws);
    float* w = reinterpret_cast<float*>(base + sp.w);
    double* partial = reinterpret_cast<double*>(base + sp.partial);
    float* share = reinterpret_cast<float*>(base + sp.share);
    int* nmin = reinterpret_cast<int*>(base + sp.nmin);
    const bool vec = d % 4 == 0 && cbl_host_aligned16(x) && cbl_host_aligned16(out) && cbl_host_aligned16(grad_out) && cbl_host_aligned16(grad_x);
    const int V = vec ? 4 : 1;
    const int DV = d / V, chunks = (DV + 255) / 256, Lmax = (DV + chunks - 1) / chunks;
    // one grid for every column chunk of the query pass (the widest chunk's trips): a workgroup without a row writes zeros, the partial rows line up
    const unsigned gq = min(cbl_round_up8(cbl_div_up(n2, IMP_BLOCK / Lmax)), (unsigned)IMP_MAX_BLOCKS);
    const unsigned gm = min(cbl_div_up(n1, IMP_BLOCK / Lmax), (unsigned)IMP_MIN_BLOCKS);
    const CblFastDiv dvK = cbl_fastdiv_make((unsigned)k);
    for (int c_0 = 0; c_0 < DV; c_0 += Lmax) {
        const int L = min(Lmax, DV - c_0);
        if (vec) {
            hipLaunchKernelGGL((imp_bwd_query_kernel<4, 4>), dim3(gq), dim3(IMP_BLOCK), 0, st, (unsigned)n2, n1, k, d, c_0, L, x, inds, keymin_d, out, grad_out, w, partial);
            hipLaunchKernelGGL((imp_min_ties_kernel<4>), dim3(gm), dim3(IMP_BLOCK), 0, st, (unsigned)n1, d, c_0, L, x, keymin_d, nmin);
        } else {
            hipLaunchKernelGGL((imp_bwd_query_kernel<1, 4>), dim3(gq), dim3(IMP_BLOCK), 0, st, (unsigned)n2, n1, k, d, c_0, L, x, inds, keymin_d, out, grad_out, w, partial);
            hipLaunchKernelGGL((imp_min_ties_kernel<1>), dim3(gm), dim3(IMP_BLOCK), 0, st, (unsigned)n1, d, c_0, L, x, keymin_d, nmin);
        }
    }
    hipLaunchKernelGGL(imp_finalize_kernel, dim3(cbl_div_up(d, IMP_FIN_COLS)), dim3(IMP_FIN_COLS * IMP_FIN_GROUPS), 0, st, d, (int)gq, (const double*)partial,
                       (int)gm, (const int*)nmin, share);
    for (int c_0 = 0; c_0 < DV; c_0 += Lmax) {
        const int L = min(Lmax, DV - c_0);
        const unsigned gt = min(cbl_round_up8(cbl_div_up(n1, IMP_BLOCK / L)), 8192u);
        if (vec)
            hipLaunchKernelGGL((imp_bwd_target_kernel<4, 2>), dim3(gt), dim3(IMP_BLOCK), 0, st, (unsigned)n1, d, c_0, L, dvK, x, keymin_d, (const float*)out, (const float*)w,
                               (const float*)share, order, inv_start, inv_src, grad_x);
        else
            hipLaunchKernelGGL((imp_bwd_target_kernel<1, 2>), dim3(gt), dim3(IMP_BLOCK), 0, st, (unsigned)n1, d, c_0, L, dvK, x, keymin_d, (const float*)out, (const float*)w,
                               (const float*)share, order, inv_start, inv_src, grad_x);
    }
    return cbl_status();
}

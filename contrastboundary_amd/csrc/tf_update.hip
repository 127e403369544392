// The TF side's parameter update over flat buffers (include/cbl_amd.h, "The TF side's parameter update"):
//   weight loss      tensorflow/models/basic_operators.py:100-130, :371-378, :444, local_aggregation_operators.py:720, build_models.py:140-145
//   per-variable clip  tensorflow/utils/average_gradients.py:21-30  (tf.clip_by_norm on every variable of a tower)
//   momentum step      tensorflow/utils/tf_graph_builder.py:99-100  (tf.train.MomentumOptimizer)
// One variable is one segment of the flat buffers; the sweeps walk CHUNKS of at most TU_CHUNK elements that never cross a segment boundary (the table is built
// once per layout, on the host: cbl_tf_update_plan).  One WAVE takes one chunk at a time: 130 variables from 72 to 2.6 M elements are ~9 000 chunks, small
// variables cost a wave trip and no launch, large ones spread over the chip.  A chunk's sum of squares is ONE fp64 partial (lanes add their elements in fp64,
// a butterfly adds the lanes), a segment's partials are added in fp64 in a fixed order by one wave: no atomics, the same bits on every call.  The apply sweep
// reads its segment's denominator once per chunk and stores every element once.  The sweeps are bound by memory: 8 B / element for the norms (4 with
// fold_decay off), 20 B / element to apply; a lane keeps four 16-byte loads per buffer in flight.
// 16-byte accesses need the addresses of all the buffers a sweep touches to agree modulo 16 (chunk begins are arbitrary): the elements before the first
// 16-byte boundary and behind the last go one by one, and a call whose buffers disagree goes one by one throughout.
#include "cbl_common.h"
#include "../../include/cbl_amd.h"

#include <limits.h>

namespace {

constexpr int TU_BLOCK = 256, TU_WAVES = TU_BLOCK / CBL_WAVE, TU_CHUNK = 2048, TU_MAX_BLOCKS = 1024, TU_BATCH = 4;

struct TuChunk { long long begin; int len; int seg; };

// chunk c of the plan: (first element, length, segment); len = 0 for a chunk the device's seg_begin does not bear out (a plan of another layout): nothing
// outside [0, total) is ever touched
__device__ __forceinline__ TuChunk tu_chunk(long long c, long long total, long long S, const long long* __restrict__ seg_begin, const int* __restrict__ plan)
{
    TuChunk k;
    k.seg = plan[S + 1 + c];
    k.begin = 0; k.len = 0;
    if (k.seg < 0 || k.seg >= S) return k;
    const long long b = seg_begin[k.seg] + (c - plan[k.seg]) * TU_CHUNK, e = min(b + (long long)TU_CHUNK, seg_begin[k.seg + 1]);
    if (c < plan[k.seg] || b < 0 || e > total || e <= b) return k;
    k.begin = b; k.len = (int)(e - b);
    return k;
}

// elements of a chunk before the first 16-byte boundary of `p + begin` (all of it when the sweep's buffers disagree modulo 16)
__device__ __forceinline__ int tu_lead(const float* p, long long begin, int len, bool vec)
{
    if (!vec) return len;
    const int lead = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p + begin) & 15u)) & 15u) >> 2);
    return lead < len ? lead : len;
}

// One wave over one chunk: body.load<V>(i) fetches element(s) i.. (V = float or float4), body.finish<V>(i, regs) computes and stores.  Whole batches of
// TU_BATCH vectors per lane are loaded before the first is finished (the loads are in flight together); the rest goes vector by vector.
template <class Body> __device__ __forceinline__ void tu_walk(const TuChunk& k, int lead, int lane, Body& body)
{
    for (int i = lane; i < lead; i += CBL_WAVE) { auto r = body.template load<float>(k.begin + i); body.template finish<float>(k.begin + i, r); }   // (< 4, or the chunk)
    const int nvec = (k.len - lead) >> 2;
    const long long v0 = k.begin + lead;
    int v = 0;
    for (; v + TU_BATCH * CBL_WAVE <= nvec; v += TU_BATCH * CBL_WAVE) {
        decltype(body.template load<float4>(0)) r[TU_BATCH];
#pragma unroll
        for (int j = 0; j < TU_BATCH; j++) r[j] = body.template load<float4>(v0 + 4ll * (v + j * CBL_WAVE + lane));
#pragma unroll
        for (int j = 0; j < TU_BATCH; j++) body.template finish<float4>(v0 + 4ll * (v + j * CBL_WAVE + lane), r[j]);
    }
    for (int u = v + lane; u < nvec; u += CBL_WAVE) { auto r = body.template load<float4>(v0 + 4ll * u); body.template finish<float4>(v0 + 4ll * u, r); }
    const int tail = lead + 4 * nvec + lane;
    if (tail < k.len) { auto r = body.template load<float>(k.begin + tail); body.template finish<float>(k.begin + tail, r); }
}

template <class V> struct TuRegs { V g, w, a; };
template <class V> __device__ __forceinline__ V tu_zero();
template <> __device__ __forceinline__ float tu_zero<float>() { return 0.f; }
template <> __device__ __forceinline__ float4 tu_zero<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }
template <class V> __device__ __forceinline__ V tu_ld(const float* p) { return *reinterpret_cast<const V*>(p); }
template <class V> __device__ __forceinline__ void tu_st(float* p, V v) { *reinterpret_cast<V*>(p) = v; }

// sum of squares of  x = g + wd * w  (GRAD, FOLD), x = g (GRAD), x = w (weight loss)
template <bool GRAD, bool FOLD> struct TuSquares {
    const float* __restrict__ params; const float* __restrict__ grads; float wd; double acc;
    template <class V> __device__ __forceinline__ TuRegs<V> load(long long i) const
    {
        TuRegs<V> r; r.a = tu_zero<V>();
        r.g = GRAD ? tu_ld<V>(grads + i) : tu_zero<V>();
        r.w = (!GRAD || FOLD) ? tu_ld<V>(params + i) : tu_zero<V>();
        return r;
    }
    template <class V> __device__ __forceinline__ void finish(long long, TuRegs<V>& r)
    {
        const float* g = reinterpret_cast<const float*>(&r.g); const float* w = reinterpret_cast<const float*>(&r.w);
#pragma unroll
        for (int j = 0; j < (int)(sizeof(V) / 4); j++) {
            const float x = !GRAD ? w[j] : FOLD ? g[j] + wd * w[j] : g[j];
            acc += (double)x * (double)x;
        }
    }
};

template <bool GRAD, bool FOLD>
__global__ __launch_bounds__(TU_BLOCK) void tf_update_squares_kernel(long long total, long long S, long long n_chunks, const float* __restrict__ params,
                                                                     const float* __restrict__ grads, const long long* __restrict__ seg_begin,
                                                                     const float* __restrict__ seg_wd, const int* __restrict__ plan, int vec,
                                                                     double* __restrict__ partial)
{
    const int lane = threadIdx.x & (CBL_WAVE - 1), wave = threadIdx.x / CBL_WAVE;
    for (long long c = (long long)blockIdx.x * TU_WAVES + wave; c < n_chunks; c += (long long)gridDim.x * TU_WAVES) {
        const TuChunk k = tu_chunk(c, total, S, seg_begin, plan);
        const float wd = (!GRAD || FOLD) && k.len ? seg_wd[k.seg] : 0.f;
        double s = 0.0;
        if (k.len && (GRAD || wd != 0.f)) {                          // the weight loss does not read an undecayed segment
            TuSquares<GRAD, FOLD> body{params, grads, wd, 0.0};
            tu_walk(k, tu_lead(GRAD ? grads : params, k.begin, k.len, vec != 0), lane, body);
            s = body.acc;
        }
        for (int m = CBL_WAVE / 2; m >= 1; m >>= 1) s += __shfl_xor(s, m);
        if (lane == 0) partial[c] = s;
    }
}

// one wave per segment: its chunks' partials, lane-strided and then a butterfly (a fixed order), in fp64
//   NORM:  norms[s] = sqrt(sum), den[s] = max(norms[s], clip_norm) — the denominator of tf.clip_by_norm
//   else:  term[s] = wd * sum / 2 (0, and nothing read, for wd = 0), seg_loss[s] its float
template <bool NORM>
__global__ __launch_bounds__(TU_BLOCK) void tf_update_segments_kernel(long long S, long long n_chunks, const int* __restrict__ plan, const double* __restrict__ partial,
                                                                      const float* __restrict__ seg_wd, float clip_norm, float* __restrict__ norms,
                                                                      float* __restrict__ den, double* __restrict__ term, float* __restrict__ seg_loss)
{
    const int lane = threadIdx.x & (CBL_WAVE - 1), wave = threadIdx.x / CBL_WAVE;
    for (long long s = (long long)blockIdx.x * TU_WAVES + wave; s < S; s += (long long)gridDim.x * TU_WAVES) {
        const float wd = NORM ? 1.f : seg_wd[s];
        double sum = 0.0;
        if (wd != 0.f)
            for (long long c = max(plan[s], 0) + lane; c < min((long long)plan[s + 1], n_chunks); c += CBL_WAVE) sum += partial[c];     // (clamped: a plan of another layout)
        for (int m = CBL_WAVE / 2; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
        if (lane != 0) continue;
        if (NORM) {
            const float norm = (float)sqrt(sum);
            norms[s] = norm;
            den[s] = fmaxf(norm, clip_norm);
        } else {
            const double t = wd != 0.f ? (double)wd * (0.5 * sum) : 0.0;
            term[s] = t;
            if (seg_loss) seg_loss[s] = (float)t;
        }
    }
}

__global__ __launch_bounds__(CBL_WAVE) void tf_update_loss_kernel(long long S, const double* __restrict__ term, float* __restrict__ loss)
{
    double sum = 0.0;
    for (long long s = threadIdx.x; s < S; s += CBL_WAVE) sum += term[s];
    for (int m = CBL_WAVE / 2; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
    if (threadIdx.x == 0) loss[0] = (float)sum;
}

// grads += coef * params  (coef = grad_loss * wd of the segment)
struct TuDecayGrad {
    const float* __restrict__ params; float* __restrict__ grads; float coef;
    template <class V> __device__ __forceinline__ TuRegs<V> load(long long i) const
    {
        TuRegs<V> r; r.a = tu_zero<V>(); r.g = tu_ld<V>(grads + i); r.w = tu_ld<V>(params + i);
        return r;
    }
    template <class V> __device__ __forceinline__ void finish(long long i, TuRegs<V>& r) const
    {
        float* g = reinterpret_cast<float*>(&r.g); const float* w = reinterpret_cast<const float*>(&r.w);
#pragma unroll
        for (int j = 0; j < (int)(sizeof(V) / 4); j++) g[j] = g[j] + coef * w[j];
        tu_st<V>(grads + i, r.g);
    }
};

__global__ __launch_bounds__(TU_BLOCK) void tf_update_decay_grad_kernel(long long total, long long S, long long n_chunks, const float* __restrict__ params,
                                                                        const long long* __restrict__ seg_begin, const float* __restrict__ seg_wd,
                                                                        const int* __restrict__ plan, int vec, const float* __restrict__ grad_loss,
                                                                        float* __restrict__ grads)
{
    const int lane = threadIdx.x & (CBL_WAVE - 1), wave = threadIdx.x / CBL_WAVE;
    const float up = grad_loss[0];
    for (long long c = (long long)blockIdx.x * TU_WAVES + wave; c < n_chunks; c += (long long)gridDim.x * TU_WAVES) {
        const TuChunk k = tu_chunk(c, total, S, seg_begin, plan);
        if (!k.len) continue;
        const float wd = seg_wd[k.seg];
        if (wd == 0.f) continue;
        TuDecayGrad body{params, grads, up * wd};
        tu_walk(k, tu_lead(grads, k.begin, k.len, vec != 0), lane, body);
    }
}

// the apply sweep:  CLIP: g' = (g + wd w) clip / den (stored);  STEP: a = momentum a + grad_scale g', w -= lr a (both stored)
template <bool CLIP, bool STEP, bool FOLD> struct TuApply {
    float* __restrict__ params; float* __restrict__ grads; float* __restrict__ accum;
    float wd, clip_norm, den, momentum, grad_scale, lr;
    template <class V> __device__ __forceinline__ TuRegs<V> load(long long i) const
    {
        TuRegs<V> r;
        r.g = tu_ld<V>(grads + i);
        r.w = (STEP || FOLD) ? tu_ld<V>(params + i) : tu_zero<V>();
        r.a = STEP ? tu_ld<V>(accum + i) : tu_zero<V>();
        return r;
    }
    template <class V> __device__ __forceinline__ void finish(long long i, TuRegs<V>& r) const
    {
        float* g = reinterpret_cast<float*>(&r.g); float* w = reinterpret_cast<float*>(&r.w); float* a = reinterpret_cast<float*>(&r.a);
#pragma unroll
        for (int j = 0; j < (int)(sizeof(V) / 4); j++) {
            if (CLIP) {
                const float h = FOLD ? g[j] + wd * w[j] : g[j];
                g[j] = clip_norm > 0.f ? (h * clip_norm) / den : h;
            }
            if (STEP) {
                a[j] = momentum * a[j] + grad_scale * g[j];
                w[j] = w[j] - lr * a[j];
            }
        }
        if (CLIP) tu_st<V>(grads + i, r.g);
        if (STEP) { tu_st<V>(accum + i, r.a); tu_st<V>(params + i, r.w); }
    }
};

template <bool CLIP, bool STEP, bool FOLD>
__global__ __launch_bounds__(TU_BLOCK) void tf_update_apply_kernel(long long total, long long S, long long n_chunks, float* __restrict__ params,
                                                                   float* __restrict__ grads, float* __restrict__ accum,
                                                                   const long long* __restrict__ seg_begin, const float* __restrict__ seg_wd,
                                                                   const int* __restrict__ seg_active, const int* __restrict__ plan, int vec,
                                                                   float clip_norm, float momentum, float grad_scale, const float* __restrict__ lr,
                                                                   const float* __restrict__ den)
{
    const int lane = threadIdx.x & (CBL_WAVE - 1), wave = threadIdx.x / CBL_WAVE;
    const float rate = STEP ? lr[0] : 0.f;
    for (long long c = (long long)blockIdx.x * TU_WAVES + wave; c < n_chunks; c += (long long)gridDim.x * TU_WAVES) {
        const TuChunk k = tu_chunk(c, total, S, seg_begin, plan);
        if (!k.len || (seg_active && !seg_active[k.seg])) continue;
        TuApply<CLIP, STEP, FOLD> body{params, grads, accum, FOLD ? seg_wd[k.seg] : 0.f, clip_norm, CLIP && clip_norm > 0.f ? den[k.seg] : 1.f,
                                       momentum, grad_scale, rate};
        tu_walk(k, tu_lead(grads, k.begin, k.len, vec != 0), lane, body);
    }
}

long long tu_max_chunks(long long total, long long S) { return total / TU_CHUNK + S; }
unsigned tu_grid(long long waves) { return cbl_grid_for(waves, TU_WAVES, TU_MAX_BLOCKS); }
// the buffers a sweep touches agree modulo 16 bytes (null = not touched)
int tu_vec(const void* a, const void* b, const void* c)
{
    const void* p[3] = {a, b, c};
    uintptr_t first = 0; bool have = false;
    for (const void* q : p) {
        if (!q) continue;
        const uintptr_t m = reinterpret_cast<uintptr_t>(q) & 15u;
        if ((m & 3u) != 0) return 0;
        if (!have) { first = m; have = true; } else if (m != first) return 0;
    }
    return 1;
}
int tu_layout_args(long long total, long long S, const long long* seg_begin, const int* plan, long long n_chunks)
{
    if (total < 0 || S < 0) return CBL_ERR_BAD_ARG;
    if (S == 0) return CBL_OK;
    if (!seg_begin || !plan || n_chunks < S || n_chunks > tu_max_chunks(total, S)) return CBL_ERR_BAD_ARG;
    if (n_chunks > INT_MAX || S > INT_MAX) return CBL_ERR_UNSUPPORTED;
    return CBL_OK;
}
size_t tu_partial_bytes(long long total, long long S) { return (size_t)tu_max_chunks(total, S) * sizeof(double); }

}  // namespace

CBL_EXPORT size_t cbl_tf_update_plan_bytes(long long total, long long S)
{
    if (total < 0 || S < 0) return 0;
    return sizeof(int) * (size_t)(S + 1 + tu_max_chunks(total, S));
}

CBL_EXPORT int cbl_tf_update_plan(long long total, long long S, const long long* seg_begin_host, void* plan_host, size_t plan_bytes, long long* n_chunks)
{
    if (total < 0 || S < 0 || !n_chunks) return CBL_ERR_BAD_ARG;
    *n_chunks = 0;
    if (S == 0) return CBL_OK;
    if (!seg_begin_host || !plan_host) return CBL_ERR_BAD_ARG;
    if (seg_begin_host[0] < 0 || seg_begin_host[S] > total) return CBL_ERR_BAD_ARG;
    long long chunks = 0;
    for (long long s = 0; s < S; s++) {
        if (seg_begin_host[s + 1] <= seg_begin_host[s]) return CBL_ERR_BAD_ARG;      // descending, or an empty segment
        chunks += (seg_begin_host[s + 1] - seg_begin_host[s] + TU_CHUNK - 1) / TU_CHUNK;
    }
    if (chunks > INT_MAX || S > INT_MAX) return CBL_ERR_UNSUPPORTED;
    if (plan_bytes < cbl_tf_update_plan_bytes(total, S)) return CBL_ERR_WORKSPACE;
    int* plan = reinterpret_cast<int*>(plan_host);
    long long c = 0;
    for (long long s = 0; s < S; s++) {
        plan[s] = (int)c;
        const long long n = (seg_begin_host[s + 1] - seg_begin_host[s] + TU_CHUNK - 1) / TU_CHUNK;
        for (long long j = 0; j < n; j++) plan[S + 1 + c + j] = (int)s;
        c += n;
    }
    plan[S] = (int)c;
    for (long long j = c; j < tu_max_chunks(total, S); j++) plan[S + 1 + j] = -1;      // never walked (n_chunks ends before them)
    *n_chunks = c;
    return CBL_OK;
}

CBL_EXPORT size_t cbl_tf_update_workspace_bytes(long long total, long long S)
{
    if (total < 0 || S < 0) return 0;
    return tu_partial_bytes(total, S) + (size_t)S * (sizeof(double) + sizeof(float)) + 256;
}

CBL_EXPORT int cbl_tf_weight_loss_forward(long long total, long long S, const float* params, const long long* seg_begin, const float* seg_wd,
                                          const int* plan, long long n_chunks, float* loss, float* seg_loss, void* workspace, size_t workspace_bytes, void* stream)
{
    const int rc = tu_layout_args(total, S, seg_begin, plan, n_chunks);
    if (rc != CBL_OK || S == 0) return rc;
    if (!params || !seg_wd || !loss || !workspace) return CBL_ERR_BAD_ARG;
    if (workspace_bytes < cbl_tf_update_workspace_bytes(total, S)) return CBL_ERR_WORKSPACE;
    hipStream_t st = cbl_stream(stream);
    double* partial = reinterpret_cast<double*>(workspace);
    double* term = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + tu_partial_bytes(total, S));
    hipLaunchKernelGGL((tf_update_squares_kernel<false, false>), dim3(tu_grid(n_chunks)), dim3(TU_BLOCK), 0, st, total, S, n_chunks, params,
                       (const float*)nullptr, seg_begin, seg_wd, plan, tu_vec(params, nullptr, nullptr), partial);
    hipLaunchKernelGGL((tf_update_segments_kernel<false>), dim3(tu_grid(S)), dim3(TU_BLOCK), 0, st, S, n_chunks, plan, (const double*)partial, seg_wd, 0.f,
                       (float*)nullptr, (float*)nullptr, term, seg_loss);
    hipLaunchKernelGGL(tf_update_loss_kernel, dim3(1), dim3(CBL_WAVE), 0, st, S, (const double*)term, loss);
    return cbl_status();
}

CBL_EXPORT int cbl_tf_weight_loss_backward(long long total, long long S, const float* params, const long long* seg_begin, const float* seg_wd,
                                           const int* plan, long long n_chunks, const float* grad_loss, float* grads, void* stream)
{
    const int rc = tu_layout_args(total, S, seg_begin, plan, n_chunks);
    if (rc != CBL_OK || S == 0) return rc;
    if (!params || !seg_wd || !grad_loss || !grads) return CBL_ERR_BAD_ARG;
    hipLaunchKernelGGL(tf_update_decay_grad_kernel, dim3(tu_grid(n_chunks)), dim3(TU_BLOCK), 0, cbl_stream(stream), total, S, n_chunks, params, seg_begin,
                       seg_wd, plan, tu_vec(params, grads, nullptr), grad_loss, grads);
    return cbl_status();
}

CBL_EXPORT int cbl_tf_clip_update(long long total, long long S, int mode, int fold_decay, float* params, float* grads, float* accum,
                                  const long long* seg_begin, const float* seg_wd, const int* seg_active, const int* plan, long long n_chunks,
                                  float clip_norm, float momentum, float grad_scale, const float* lr, float* norms,
                                  void* workspace, size_t workspace_bytes, void* stream)
{
    if (mode < 1 || mode > (CBL_TF_UPDATE_CLIP | CBL_TF_UPDATE_STEP)) return CBL_ERR_BAD_ARG;
    const int rc = tu_layout_args(total, S, seg_begin, plan, n_chunks);
    if (rc != CBL_OK || S == 0) return rc;
    const bool clip = (mode & CBL_TF_UPDATE_CLIP) != 0, step = (mode & CBL_TF_UPDATE_STEP) != 0, fold = clip && fold_decay != 0;
    if (!grads) return CBL_ERR_BAD_ARG;
    if (clip && (!norms || !workspace || (fold && (!params || !seg_wd)))) return CBL_ERR_BAD_ARG;
    if (step && (!params || !accum || !lr)) return CBL_ERR_BAD_ARG;
    if (clip && workspace_bytes < cbl_tf_update_workspace_bytes(total, S)) return CBL_ERR_WORKSPACE;
    hipStream_t st = cbl_stream(stream);
    const dim3 grid(tu_grid(n_chunks)), block(TU_BLOCK);
    float* den = nullptr;
    if (clip) {
        double* partial = reinterpret_cast<double*>(workspace);
        den = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + tu_partial_bytes(total, S) + (size_t)S * sizeof(double));
        const int vec = tu_vec(grads, fold ? params : nullptr, nullptr);
        if (fold)
            hipLaunchKernelGGL((tf_update_squares_kernel<true, true>), grid, block, 0, st, total, S, n_chunks, (const float*)params, (const float*)grads,
                               seg_begin, seg_wd, plan, vec, partial);
        else
            hipLaunchKernelGGL((tf_update_squares_kernel<true, false>), grid, block, 0, st, total, S, n_chunks, (const float*)params, (const float*)grads,
                               seg_begin, seg_wd, plan, vec, partial);
        hipLaunchKernelGGL((tf_update_segments_kernel<true>), dim3(tu_grid(S)), block, 0, st, S, n_chunks, plan, (const double*)partial, seg_wd, clip_norm, norms, den,
                           (double*)nullptr, (float*)nullptr);
    }
    const int vec = tu_vec(grads, (step || fold) ? params : nullptr, step ? accum : nullptr);
#define TU_APPLY(C, T, F)                                                                                                                                   \
    hipLaunchKernelGGL((tf_update_apply_kernel<C, T, F>), grid, block, 0, st, total, S, n_chunks, params, grads, accum, seg_begin, seg_wd, seg_active, plan, \
                       vec, clip_norm, momentum, grad_scale, lr, (const float*)den)
    if (clip && step) { if (fold) TU_APPLY(true, true, true); else TU_APPLY(true, true, false); }
    else if (clip) { if (fold) TU_APPLY(true, false, true); else TU_APPLY(true, false, false); }
    else TU_APPLY(false, true, false);
#undef TU_APPLY
    return cbl_status();
}

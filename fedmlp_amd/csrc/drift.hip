// Client-drift correction of the gradient an optimizer step reads (FedProx's proximal term, SCAFFOLD's control-variate shift and
// the running sum of raw gradients its new control variate is made of): one streaming launch over the trainable arena, enqueued
// in front of the optimizer kernel only while a correction is installed (engine.hip: drift_grad).  gfx950.
//
// Operands, all in arena layout (NP floats, NP a multiple of 4): the raw gradient g (read only), the student's parameters p, the
// anchor a (the parameters at fm_drift_begin), the shift s, the running sum S and the output r, which the optimizer kernel then
// reads in g's place.  Per element, in fp32, every operation rounded on its own (`fp contract(off)`, as fedavg_fold_kernel):
//     r = g
//     PROX  :  d = p - a;  m = mu * d;  r = r + m
//     SHIFT :  r = r + s
//     TRACK :  S = S + g            (the raw gradient)
// Which of the three terms a launch carries is a template argument: a FedProx launch neither reads nor names s and S.
// Bytes moved per parameter: 8 (g, r) + 8 (PROX) + 4 (SHIFT) + 8 (TRACK), 28 with everything on -- the Adam launch's traffic.
// Like the optimizer kernels it takes the engine's skip word (a lost stream-K part poisoned g: nothing is written, and the
// optimizer behind it does nothing either) and never synchronises with the host.
#include "common.h"
#include "kernels.h"

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

template <bool PROX, bool SHIFT, bool TRACK>
struct DriftRule {
    DriftOps a;
    struct Hp {};             // the scalars travel with the operands
    struct Quad { f32x4 g, p, a, s, S, r; };
    __device__ __forceinline__ void load(Quad& q, int64_t o) const
    {
        q.g = *reinterpret_cast<const f32x4*>(a.g + o);
        if (PROX) { q.p = *reinterpret_cast<const f32x4*>(a.p + o); q.a = *reinterpret_cast<const f32x4*>(a.a + o); }
        if (SHIFT) q.s = *reinterpret_cast<const f32x4*>(a.s + o);
        if (TRACK) q.S = *reinterpret_cast<const f32x4*>(a.S + o);
    }
    __device__ __forceinline__ void update(Quad& q, const Hp& = Hp{}) const
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float r = q.g[k];
            if (PROX) {
                const float d = q.p[k] - q.a[k];
                const float m = a.mu * d;
                r = r + m;
            }
            if (SHIFT) r = r + q.s[k];
            if (TRACK) q.S[k] = q.S[k] + q.g[k];
            q.r[k] = r;
        }
    }
    __device__ __forceinline__ void store(const Quad& q, int64_t o, int64_t begin, int64_t end) const
    {
        store_own(a.r, o, begin, end, q.r);
        if (TRACK) store_own(a.S, o, begin, end, q.S);
    }
};

// ---- the flat form: [0, 4 n4), no requires_grad mask.  Block b owns the ARENA_QPT * 256 quads from b * ARENA_QPT * 256 on;
// thread t takes quads t, t + 256, ...; all its 16-byte loads are in flight before the first use
template <bool PROX, bool SHIFT, bool TRACK>
__global__ void __launch_bounds__(256) drift_flat_kernel(const DriftRule<PROX, SHIFT, TRACK> r, int64_t n4, const int* __restrict__ skip)
{
    if (skip && *skip) return;
    const int64_t i0 = (int64_t)blockIdx.x * (ARENA_QPT * 256) + threadIdx.x;
    typename DriftRule<PROX, SHIFT, TRACK>::Quad q[ARENA_QPT];
#pragma unroll
    for (int j = 0; j < ARENA_QPT; ++j) {
        const int64_t i = i0 + (int64_t)j * 256;
        if (i < n4) r.load(q[j], 4 * i);
    }
#pragma unroll
    for (int j = 0; j < ARENA_QPT; ++j) {
        const int64_t i = i0 + (int64_t)j * 256;
        if (i < n4) {
            r.update(q[j]);
            *reinterpret_cast<f32x4*>(r.a.r + 4 * i) = q[j].r;
            if (TRACK) *reinterpret_cast<f32x4*>(r.a.S + 4 * i) = q[j].S;
        }
    }
}

// ---- the table form: one block per parameter chunk of the engine's entry / chunk table (arena_table.h), under a
// requires_grad mask.  sel = 0 marks a trainable entry: corrected and tracked with the flat form's arithmetic, arena_walk's
// boundary rule (whole quads read, own floats written).  Anything else is a frozen one: r = 0 over its span, S untouched, no
// load.  Floats outside every entry are touched by nobody and stay the zeros r and S were allocated with.
template <bool PROX, bool SHIFT, bool TRACK>
__global__ void __launch_bounds__(256) drift_masked_kernel(const DriftRule<PROX, SHIFT, TRACK> r, const ArenaChunk* __restrict__ chunks,
                                                           const OptSel sel, const int* __restrict__ skip)
{
    if (skip && *skip) return;
    const ArenaChunk ch = chunks[blockIdx.x];
    if (opt_sel_get(sel, ch.ent) != 0u) {
        const int64_t begin = ch.begin, end = begin + ch.len;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        for (int64_t o = (begin & ~(int64_t)3) + 4 * (int64_t)threadIdx.x; o < end; o += 1024) store_own(r.a.r, o, begin, end, z);
        return;
    }
    arena_walk(r, ch, {});
}

template <bool PROX, bool SHIFT, bool TRACK>
static void drift_launch(const DriftOps& a, int64_t n, const ArenaChunk* chunks, int n_chunks, const OptSel* sel, hipStream_t s,
                         const int* skip)
{
    const DriftRule<PROX, SHIFT, TRACK> r{a};
    if (!chunks) {
        const int64_t n4 = n / 4;
        hipLaunchKernelGGL((drift_flat_kernel<PROX, SHIFT, TRACK>), dim3(cdiv(n4, ARENA_QPT * 256)), dim3(256), 0, s, r, n4, skip);
    } else {
        hipLaunchKernelGGL((drift_masked_kernel<PROX, SHIFT, TRACK>), dim3(n_chunks), dim3(256), 0, s, r, chunks, *sel, skip);
    }
}
template <bool PROX, bool SHIFT>
static void drift_launch_t(const DriftOps& a, int64_t n, const ArenaChunk* chunks, int n_chunks, const OptSel* sel, hipStream_t s,
                           const int* skip)
{
    if (a.S) drift_launch<PROX, SHIFT, true>(a, n, chunks, n_chunks, sel, s, skip);
    else drift_launch<PROX, SHIFT, false>(a, n, chunks, n_chunks, sel, s, skip);
}
static void drift_dispatch(const DriftOps& a, int64_t n, const ArenaChunk* chunks, int n_chunks, const OptSel* sel, hipStream_t s,
                           const int* skip)
{
    const bool prox = a.mu != 0.f, shift = a.s != nullptr;
    if (prox && shift) drift_launch_t<true, true>(a, n, chunks, n_chunks, sel, s, skip);
    else if (prox) drift_launch_t<true, false>(a, n, chunks, n_chunks, sel, s, skip);
    else if (shift) drift_launch_t<false, true>(a, n, chunks, n_chunks, sel, s, skip);
    else drift_launch_t<false, false>(a, n, chunks, n_chunks, sel, s, skip);
}

void k_drift_correct(const DriftOps& a, int64_t n, hipStream_t s, const int* skip)
{
    drift_dispatch(a, n, nullptr, 0, nullptr, s, skip);
}
void k_drift_correct_masked(const DriftOps& a, const ArenaChunk* chunks, int n_chunks, const OptSel& sel, hipStream_t s, const int* skip)
{
    drift_dispatch(a, 0, chunks, n_chunks, &sel, s, skip);
}

// x[i] = x[i] / k for n floats at any alignment (fm_drift_end: the mean of the round's raw gradients, S / (float)K, one IEEE
// division per element)
__global__ void drift_div_kernel(float* __restrict__ x, float k, int64_t n)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[i] = x[i] / k;
}
void k_drift_div(float* x, float k, int64_t n, hipStream_t s)
{
    if (n > 0) hipLaunchKernelGGL(drift_div_kernel, dim3((unsigned)std::min<int64_t>(cdiv(n, 256), 8192)), dim3(256), 0, s, x, k, n);
}

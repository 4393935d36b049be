// Optimizer kernels of the autograd path over the engine's flat arenas (weights, gradient accumulator, moments: NP floats each,
// NP a multiple of 4): torch.optim.SGD, torch.optim.AdamW, the L2 norm of the accumulator and the two clips.  gfx950.
//
// All of them stream the arena once in 16-byte elements on the main lane's stream, take the engine's skip word (a kernel of
// this step reported a lost part: nothing is written, like adam_kernel in elementwise.hip) and never synchronise with the host.
// The element-wise ones run one 16-byte element per thread (k_bn_bwd_apply's launcher has the measurement); Adam with coupled
// L2 stays where it was (adam_kernel, elementwise.hip), untouched, so the fused steps keep their code.
// Bytes moved per parameter: SGD 12 (no momentum) / 20, AdamW 28, norm 4, clip 8.
#include "common.h"
#include "kernels.h"

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// ------------------------------------------------------------------ SGD --------
// torch.optim.SGD's single-tensor update in its order: g += wd p; buf = g (first step after a reset) or momentum buf +
// (1 - dampening) g; g = nesterov ? g + momentum buf : buf; p -= lr g.
// MODE 0: momentum = 0, the buffer is neither read nor written; 1: first step (buf = g, no dampening: torch clones the
// gradient); 2: every later step.
// The chain is evaluated in double from the fp32 operands and each stored value (buf, p) is rounded once.  In fp32 the new p
// would inherit the rounding of momentum buf + (1 - dampening) g, half an ulp of its OPERANDS: where the two terms cancel and p is
// small against lr buf that is many ulps of p (tests/test_optim_gpu.py's bound, 4 ulp(p) + 1e-5 |dp|, is missed by a pure fp32
// chain, torch's own included).  Five double operations per parameter beside 12 / 20 bytes of HBM traffic: still a streaming kernel.
template <int MODE>
__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, int64_t n4, double lr,
                           double momentum, double one_minus_damp, double wd, int nesterov, const int* __restrict__ skip)
{
    if (skip && *skip) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
    const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
    f32x4 bb = {0.f, 0.f, 0.f, 0.f};
    if (MODE == 2) bb = reinterpret_cast<const f32x4*>(buf)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double d = (double)gg[k] + wd * (double)pp[k];
        if (MODE != 0) {
            const double b = MODE == 1 ? d : momentum * (double)bb[k] + one_minus_damp * d;
            bb[k] = (float)b;
            d = nesterov ? d + momentum * b : b;
        }
        pp[k] = (float)((double)pp[k] - lr * d);
    }
    if (MODE != 0) reinterpret_cast<f32x4*>(buf)[i] = bb;
    reinterpret_cast<f32x4*>(p)[i] = pp;
}
void k_sgd(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, double one_minus_damp, float wd,
           bool nesterov, bool first, hipStream_t s, const int* skip)
{
    const int64_t n4 = n / 4;
    const dim3 grid(cdiv(n4, 256)), block(256);
    const double lr_ = lr, mom = momentum, wd_ = wd;
    if (momentum == 0.f)
        hipLaunchKernelGGL(sgd_kernel<0>, grid, block, 0, s, p, g, buf, n4, lr_, mom, one_minus_damp, wd_, 0, skip);
    else if (first)
        hipLaunchKernelGGL(sgd_kernel<1>, grid, block, 0, s, p, g, buf, n4, lr_, mom, one_minus_damp, wd_, nesterov ? 1 : 0, skip);
    else
        hipLaunchKernelGGL(sgd_kernel<2>, grid, block, 0, s, p, g, buf, n4, lr_, mom, one_minus_damp, wd_, nesterov ? 1 : 0, skip);
}

// ---------------------------------------------------------------- AdamW --------
// torch.optim.AdamW's single-tensor update in its order: p *= 1 - lr wd; exp_avg.lerp_(g, 1 - beta1); exp_avg_sq = beta2
// exp_avg_sq + (1 - beta2) g g; denom = sqrt(exp_avg_sq) / sqrt(bc2) + eps; p -= lr / bc1 * exp_avg / denom.  No L2 in g.
// decay = 1 - lr wd and step = lr / bc1 are formed on the host in double.
__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                             int64_t n4, float decay, float step, double one_minus_b1, float b2, float eps, float bc2_sqrt,
                             const int* __restrict__ skip)
{
    if (skip && *skip) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    f32x4 pp = reinterpret_cast<f32x4*>(p)[i] * decay;
    const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
    f32x4 mm = reinterpret_cast<f32x4*>(m)[i];
    f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
    vv = vv * b2 + (1.f - b2) * gg * gg;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // the lerp in double, rounded once: where beta1 m and (1 - beta1) g cancel, an fp32 lerp is half an ulp of its OPERANDS
        // off, and lr / bc1 times that over denom is many ulps of a small p (the SGD kernel's note); everything after it carries
        // errors relative to the update itself and stays in fp32
        mm[k] = (float)((double)mm[k] + one_minus_b1 * ((double)gg[k] - (double)mm[k]));
        const float den = sqrtf(vv[k]) / bc2_sqrt + eps;
        pp[k] = pp[k] - step * (mm[k] / den);
    }
    reinterpret_cast<f32x4*>(p)[i] = pp;
    reinterpret_cast<f32x4*>(m)[i] = mm;
    reinterpret_cast<f32x4*>(v)[i] = vv;
}
void k_adamw(float* p, const float* g, float* m, float* v, int64_t n, float decay, float step, float b1, float b2, float eps,
             float bc2_sqrt, hipStream_t s, const int* skip)
{
    const int64_t n4 = n / 4;
    hipLaunchKernelGGL(adamw_kernel, dim3(cdiv(n4, 256)), dim3(256), 0, s, p, g, m, v, n4, decay, step, 1.0 - (double)b1, b2, eps, bc2_sqrt, skip);
}

// ------------------------------------------------------------- L2 norm ---------
// Deterministic (no atomics), two launches.  Stage 1: block b of 256 threads owns the GRAD_NORM_F4 * 256 16-byte elements from
// b * GRAD_NORM_F4 * 256 on; thread t reads elements t, t + 256, ... (all loads in flight before the first use), squares and
// adds them into one fp32 accumulator per vector component -- GRAD_NORM_F4 serial additions -- adds the four components as
// (0 + 1) + (2 + 3), and the block sums its 256 values in a fixed tree: xor-shuffles over the 64 lanes (6 levels), then the
// four waves through LDS as (w0 + w1) + (w2 + w3).  The block's sum leaves fp32 here: part[b] is a double.
// Stage 2: ONE block; thread t adds part[t], part[t + 256], ... in double, in that order, the 256 sums are folded in LDS in a
// fixed halving tree, and thread 0 writes sqrtf of the total as one float.
// Elements past n4 (the last block's tail) read as zero.  The engine's padding inside the arena holds exact zeros.
__global__ void __launch_bounds__(256) grad_sqsum_kernel(const float* __restrict__ g, int64_t n4, double* __restrict__ part,
                                                         const int* __restrict__ skip)
{
    if (skip && *skip) return;
    __shared__ float wsum[4];
    const int64_t base = (int64_t)blockIdx.x * (GRAD_NORM_F4 * 256) + threadIdx.x;
    f32x4 v[GRAD_NORM_F4];
#pragma unroll
    for (int j = 0; j < GRAD_NORM_F4; ++j) {
        const int64_t i = base + (int64_t)j * 256;
        v[j] = i < n4 ? reinterpret_cast<const f32x4*>(g)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < GRAD_NORM_F4; ++j) acc = acc + v[j] * v[j];
    float s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (double)((wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));
}
__global__ void __launch_bounds__(256) grad_norm_final_kernel(const double* __restrict__ part, int nparts, float* __restrict__ norm,
                                                              const int* __restrict__ skip)
{
    if (skip && *skip) return;
    __shared__ double sm[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) s += part[i];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *norm = sqrtf((float)sm[0]);
}
int grad_norm_parts(int64_t n) { return cdiv(n / 4, (int64_t)GRAD_NORM_F4 * 256); }
void k_grad_norm(const float* g, int64_t n, double* part, float* norm, hipStream_t s, const int* skip)
{
    const int nparts = grad_norm_parts(n);
    hipLaunchKernelGGL(grad_sqsum_kernel, dim3(nparts), dim3(256), 0, s, g, n / 4, part, skip);
    hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(256), 0, s, part, nparts, norm, skip);
}

// ---------------------------------------------------------------- clips --------
// torch.nn.utils.clip_grad_norm_: g *= min(1, max_norm / (norm + 1e-6)), the coefficient formed in fp32 from the device word;
// the multiply always happens and a non-finite norm propagates (a NaN coefficient is not clamped, like torch.clamp).
__global__ void grad_clip_norm_kernel(float* __restrict__ g, int64_t n4, const float* __restrict__ norm, float max_norm,
                                      const int* __restrict__ skip)
{
    if (skip && *skip) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float c = max_norm / (*norm + 1e-6f);
    c = c > 1.f ? 1.f : c;
    reinterpret_cast<f32x4*>(g)[i] = reinterpret_cast<const f32x4*>(g)[i] * c;
}
void k_grad_clip_norm(float* g, int64_t n, const float* norm, float max_norm, hipStream_t s, const int* skip)
{
    const int64_t n4 = n / 4;
    hipLaunchKernelGGL(grad_clip_norm_kernel, dim3(cdiv(n4, 256)), dim3(256), 0, s, g, n4, norm, max_norm, skip);
}

// torch.nn.utils.clip_grad_value_: g = clamp(g, -clip, clip); a NaN stays a NaN
__global__ void grad_clip_value_kernel(float* __restrict__ g, int64_t n4, float clip, const int* __restrict__ skip)
{
    if (skip && *skip) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    f32x4 x = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = x[k] < -clip ? -clip : (x[k] > clip ? clip : x[k]);
    reinterpret_cast<f32x4*>(g)[i] = x;
}
void k_grad_clip_value(float* g, int64_t n, float clip, hipStream_t s, const int* skip)
{
    const int64_t n4 = n / 4;
    hipLaunchKernelGGL(grad_clip_value_kernel, dim3(cdiv(n4, 256)), dim3(256), 0, s, g, n4, clip, skip);
}

// ------------------------------------------- parameter groups, frozen entries --------
// The three steps again, over the entry table of the trainable arena (engine.hip: ensure_opt_table) instead of the flat arena:
// one block of 256 threads per chunk of <= FM_DIST_CHUNK floats of ONE state entry, whose parameter group the block fetches
// once from the launch's own argument block (OptSel: four bits per entry).  An entry nobody steps -- in no group, or frozen --
// costs its blocks one kernel-argument read: they return before any load.  The hyper-parameters are an argument array of
// OPT_MAX_GROUPS structs holding what the single-group launchers pass to their kernels, formed the same way on the host.
//
// An entry begins at any element offset, so a chunk's first quad starts at the 16-byte boundary at or below `begin`
// (state_dist_kernel's rule) and that quad -- like the last one -- may hold floats of the neighbouring entry, which belongs to
// another block and possibly to another group or to nobody.  A block therefore WRITES only its own floats: the first and the
// last quad of a chunk are stored lane by lane (4-byte stores of the lanes inside [begin, end)), interior quads as 16 bytes.  It
// still reads and computes whole quads: the neighbour's lanes are computed and dropped.  Floats outside every entry (the gaps
// between matrices and vectors, a padded BatchNorm vector's tail) are touched by nobody and stay zero; padding inside an entry's
// span (padded input channels and taps, the packed stem's row tails) is stepped with its entry and stays zero under all three
// rules (zero weight, zero gradient: DESIGN.md section 1's padding note).
//
// The arithmetic per element is adam_kernel's (elementwise.hip), adamw_kernel's and sgd_kernel<MODE>'s above, restated: Adam
// and SGD on the same expressions, which the compiler contracts alike in both kernels; AdamW with its contraction spelled out
// (AdamWRule).  tests/test_param_groups_gpu.py compares the bits of every pair.
// A thread holds OPT_QPT quads of every operand: all its 16-byte loads are in flight before the first use.  A full chunk that
// starts off a 16-byte boundary has one quad more (2049): thread 0 takes it after the others.
#define OPT_QPT (FM_DIST_CHUNK / 4 / 256)

__device__ __forceinline__ unsigned opt_sel_get(const OptSel& t, int ent) { return (t.w[ent >> 3] >> ((ent & 7) * 4)) & 15u; }

__device__ __forceinline__ void store_own(float* __restrict__ a, int64_t o, int64_t begin, int64_t end, const f32x4 v)
{
    if (o >= begin && o + 4 <= end) {
        *reinterpret_cast<f32x4*>(a + o) = v;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (o + k >= begin && o + k < end) a[o + k] = v[k];
    }
}

struct AdamRule {
    float* p; const float* g; float* m; float* v;
    OptAdamArgs a;
    struct Quad { f32x4 p, g, m, v; };
    __device__ __forceinline__ void load(Quad& q, int64_t o, unsigned) const
    {
        q.p = *reinterpret_cast<const f32x4*>(p + o); q.g = *reinterpret_cast<const f32x4*>(g + o);
        q.m = *reinterpret_cast<const f32x4*>(m + o); q.v = *reinterpret_cast<const f32x4*>(v + o);
    }
    __device__ __forceinline__ void update(Quad& q, unsigned gi) const
    {
        const float lr = a.hp[gi].lr, b1 = a.hp[gi].b1, b2 = a.hp[gi].b2, eps = a.hp[gi].eps, wd = a.hp[gi].wd;
        const float bc1 = a.hp[gi].bc1, bc2_sqrt = a.hp[gi].bc2_sqrt;
        const float step = lr / bc1;
        f32x4 pp = q.p;
        f32x4 gg = q.g + wd * pp;
        f32x4 mm = q.m;
        f32x4 vv = q.v;
        mm = mm + (1.f - b1) * (gg - mm);
        vv = vv * b2 + (1.f - b2) * gg * gg;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float den = sqrtf(vv[k]) / bc2_sqrt + eps;
            pp[k] = pp[k] - step * (mm[k] / den);
        }
        q.p = pp; q.m = mm; q.v = vv;
    }
    __device__ __forceinline__ void store(const Quad& q, int64_t o, int64_t begin, int64_t end, unsigned) const
    {
        store_own(p, o, begin, end, q.p); store_own(m, o, begin, end, q.m); store_own(v, o, begin, end, q.v);
    }
};

struct AdamWRule {
    float* p; const float* g; float* m; float* v;
    OptAdamWArgs a;
    struct Quad { f32x4 p, g, m, v; };
    __device__ __forceinline__ void load(Quad& q, int64_t o, unsigned) const
    {
        q.p = *reinterpret_cast<const f32x4*>(p + o); q.g = *reinterpret_cast<const f32x4*>(g + o);
        q.m = *reinterpret_cast<const f32x4*>(m + o); q.v = *reinterpret_cast<const f32x4*>(v + o);
    }
    __device__ __forceinline__ void update(Quad& q, unsigned gi) const
    {
#pragma clang fp contract(off)
        const float decay = a.hp[gi].decay, step = a.hp[gi].step, b2 = a.hp[gi].b2, eps = a.hp[gi].eps;
        const float bc2_sqrt = a.hp[gi].bc2_sqrt;
        const double one_minus_b1 = a.hp[gi].one_minus_b1;
        // adamw_kernel's expressions leave the compiler three choices of what to contract (which product of the exp_avg_sq
        // update joins the addition, and whether p * decay or step * (m / denom) joins the subtraction), and it does not make them
        // alike in two kernels.  So the choices adamw_kernel's code object holds are spelled out here with contraction off:
        //   exp_avg_sq = fma(g, (1 - beta2) g, exp_avg_sq beta2);   p = fma(decay, p, -(step (exp_avg / denom)))
        // and the lerp as there, one fma in double.  tests/test_param_groups_gpu.py holds the two kernels to the same bits.
        f32x4 pp = q.p;
        const f32x4 gg = q.g;
        f32x4 mm = q.m;
        f32x4 vv = q.v;
        const float one_minus_b2 = 1.f - b2, nstep = -step;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            vv[k] = __builtin_fmaf(gg[k], one_minus_b2 * gg[k], vv[k] * b2);
            mm[k] = (float)__builtin_fma(one_minus_b1, (double)gg[k] - (double)mm[k], (double)mm[k]);
            const float den = sqrtf(vv[k]) / bc2_sqrt + eps;
            pp[k] = __builtin_fmaf(decay, pp[k], nstep * (mm[k] / den));       // (-step) x = -(step x), signed zeros included
        }
        q.p = pp; q.m = mm; q.v = vv;
    }
    __device__ __forceinline__ void store(const Quad& q, int64_t o, int64_t begin, int64_t end, unsigned) const
    {
        store_own(p, o, begin, end, q.p); store_own(m, o, begin, end, q.m); store_own(v, o, begin, end, q.v);
    }
};

template <int MODE>
__device__ __forceinline__ void sgd_quad(f32x4& pp, const f32x4 gg, f32x4& bb, double lr, double momentum, double one_minus_damp,
                                         double wd, int nesterov)
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double d = (double)gg[k] + wd * (double)pp[k];
        if (MODE != 0) {
            const double b = MODE == 1 ? d : momentum * (double)bb[k] + one_minus_damp * d;
            bb[k] = (float)b;
            d = nesterov ? d + momentum * b : b;
        }
        pp[k] = (float)((double)pp[k] - lr * d);
    }
}
// MODE is a template argument here too: one instantiation of the whole chunk loop per MODE, chosen by the block from its group's
// mode, so that each keeps sgd_kernel<MODE>'s expression tree (a run-time MODE inside the loop lets the compiler merge the three)
template <int MODE>
struct SgdRule {
    float* p; const float* g; float* buf;
    const OptSgdArgs& a;
    struct Quad { f32x4 p, g, b; };
    __device__ __forceinline__ void load(Quad& q, int64_t o, unsigned) const
    {
        q.p = *reinterpret_cast<const f32x4*>(p + o); q.g = *reinterpret_cast<const f32x4*>(g + o);
        q.b = f32x4{0.f, 0.f, 0.f, 0.f};
        if (MODE == 2) q.b = *reinterpret_cast<const f32x4*>(buf + o);
    }
    __device__ __forceinline__ void update(Quad& q, unsigned gi) const
    {
        sgd_quad<MODE>(q.p, q.g, q.b, a.hp[gi].lr, a.hp[gi].momentum, a.hp[gi].one_minus_damp, a.hp[gi].wd, a.hp[gi].nesterov);
    }
    __device__ __forceinline__ void store(const Quad& q, int64_t o, int64_t begin, int64_t end, unsigned) const
    {
        if (MODE != 0) store_own(buf, o, begin, end, q.b);
        store_own(p, o, begin, end, q.p);
    }
};

template <class R>
__device__ __forceinline__ void opt_chunk(const R& r, const OptChunk ch, unsigned gi)
{
    const int64_t begin = ch.begin, end = begin + ch.len;
    const int64_t o0 = (begin & ~(int64_t)3) + 4 * (int64_t)threadIdx.x;
    typename R::Quad q[OPT_QPT];
#pragma unroll
    for (int j = 0; j < OPT_QPT; ++j) {
        const int64_t o = o0 + (int64_t)j * 1024;
        if (o < end) r.load(q[j], o, gi);
    }
#pragma unroll
    for (int j = 0; j < OPT_QPT; ++j) {
        const int64_t o = o0 + (int64_t)j * 1024;
        if (o < end) {
            r.update(q[j], gi);
            r.store(q[j], o, begin, end, gi);
        }
    }
    const int64_t o = o0 + (int64_t)OPT_QPT * 1024;
    if (o < end) {
        typename R::Quad t;
        r.load(t, o, gi);
        r.update(t, gi);
        r.store(t, o, begin, end, gi);
    }
}
template <class R>
__global__ void __launch_bounds__(256) opt_groups_kernel(const R r, const OptChunk* __restrict__ chunks, const OptSel sel,
                                                         const int* __restrict__ skip)
{
    if (skip && *skip) return;
    const OptChunk ch = chunks[blockIdx.x];
    const unsigned gi = opt_sel_get(sel, ch.ent);
    if (gi >= OPT_MAX_GROUPS) return;             // in no group, or frozen: before any load
    opt_chunk(r, ch, gi);
}
__global__ void __launch_bounds__(256) sgd_groups_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                         const OptSgdArgs a, const OptChunk* __restrict__ chunks, const OptSel sel,
                                                         const int* __restrict__ skip)
{
    if (skip && *skip) return;
    const OptChunk ch = chunks[blockIdx.x];
    const unsigned gi = opt_sel_get(sel, ch.ent);
    if (gi >= OPT_MAX_GROUPS) return;
    const int mode = a.hp[gi].mode;
    if (mode == 0) opt_chunk(SgdRule<0>{p, g, buf, a}, ch, gi);
    else if (mode == 1) opt_chunk(SgdRule<1>{p, g, buf, a}, ch, gi);
    else opt_chunk(SgdRule<2>{p, g, buf, a}, ch, gi);
}

void k_adam_groups(float* p, const float* g, float* m, float* v, const OptChunk* chunks, int n_chunks, const OptSel& sel,
                   const OptAdamArgs& a, hipStream_t s, const int* skip)
{
    const AdamRule r{p, g, m, v, a};
    hipLaunchKernelGGL(opt_groups_kernel<AdamRule>, dim3(n_chunks), dim3(256), 0, s, r, chunks, sel, skip);
}
void k_adamw_groups(float* p, const float* g, float* m, float* v, const OptChunk* chunks, int n_chunks, const OptSel& sel,
                    const OptAdamWArgs& a, hipStream_t s, const int* skip)
{
    const AdamWRule r{p, g, m, v, a};
    hipLaunchKernelGGL(opt_groups_kernel<AdamWRule>, dim3(n_chunks), dim3(256), 0, s, r, chunks, sel, skip);
}
void k_sgd_groups(float* p, const float* g, float* buf, const OptChunk* chunks, int n_chunks, const OptSel& sel,
                  const OptSgdArgs& a, hipStream_t s, const int* skip)
{
    hipLaunchKernelGGL(sgd_groups_kernel, dim3(n_chunks), dim3(256), 0, s, p, g, buf, a, chunks, sel, skip);
}

// k_grad_accumulate under a mask, over the same table with the same boundary rule: sel = 0 marks a trainable entry (acc = g or
// acc += g, the flat kernel's one addition), anything else a frozen one, whose span becomes exact zeros in both forms -- whatever
// e->grad holds there (a skipped weight gradient leaves it stale).
__global__ void __launch_bounds__(256) grad_accumulate_masked_kernel(float* __restrict__ acc, const float* __restrict__ g,
                                                                     const OptChunk* __restrict__ chunks, const OptSel sel, int copy,
                                                                     const int* __restrict__ skip)
{
    if (skip && *skip) return;
    const OptChunk ch = chunks[blockIdx.x];
    const bool frozen = opt_sel_get(sel, ch.ent) != 0u;
    const int64_t begin = ch.begin, end = begin + ch.len;
    for (int64_t o = (begin & ~(int64_t)3) + 4 * (int64_t)threadIdx.x; o < end; o += 1024) {
        f32x4 r = {0.f, 0.f, 0.f, 0.f};
        if (!frozen) {
            const f32x4 gg = *reinterpret_cast<const f32x4*>(g + o);
            r = copy ? gg : *reinterpret_cast<const f32x4*>(acc + o) + gg;
        }
        store_own(acc, o, begin, end, r);
    }
}
void k_grad_accumulate_masked(float* acc, const float* g, const OptChunk* chunks, int n_chunks, const OptSel& sel, bool copy,
                              hipStream_t s, const int* skip)
{
    hipLaunchKernelGGL(grad_accumulate_masked_kernel, dim3(n_chunks), dim3(256), 0, s, acc, g, chunks, sel, copy ? 1 : 0, skip);
}

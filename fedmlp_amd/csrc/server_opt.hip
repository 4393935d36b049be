// Server optimizers of the Adaptive Federated Optimization family (Reddi et al., ICLR 2021: FedAvgM, FedAdagrad, FedAdam,
// FedYogi): one streaming launch over the parameters of the engine's state, enqueued by fm_server_opt_step only
// (include/fedmlp_hip_server.h).  gfx950.
//
// Operands in engine layout: x the global model the round started from (read only, the caller's buffer), a the aggregated model
// (the engine's state: x' is written over it), m and v the two server moments (NP floats each, in place).  Per element, in fp32,
// every operation rounded on its own (`fp contract(off)`, as drift.hip), IEEE division and square root:
//     d  = a - x
//     m  : AVGM     m = beta1*m + d
//          others   t = beta1*m ; u = omb1*d ; m = t + u
//     v  : ADAGRAD  q = d*d ; v = v + q
//          ADAM     q = d*d ; t = beta2*v ; u = omb2*q ; v = t + u
//          YOGI     q = d*d ; s = sign(v - q) (sign(0) = 0) ; u = omb2*q ; u = u*s ; v = v - u
//     x' : AVGM     t = lr*m ; x' = x + t
//          others   r = sqrt(v) ; r = r + tau ; t = lr*m ; t = t / r ; x' = x + t
// The rule is a template argument: an AVGM launch neither reads nor names v.  Bytes moved per parameter: 28 (x, a, m, v read;
// x', m, v written), 20 for AVGM.  The BatchNorm running statistics behind NP are the aggregate's and stay where they are: the
// launch works in place, so x' = a there is no traffic at all.
//
// Grid: one block of 256 threads per parameter chunk of the engine's entry / chunk table (arena_table.h: <= FM_DIST_CHUNK
// floats of ONE state entry, arena_walk's boundary rule -- whole quads read, own floats written).  Padding inside an entry's
// span (a == x == 0) is stepped like any element and stays an exact zero: d = 0, m = 0, t = 0 (r >= tau > 0).  Floats outside
// every span are touched by nobody.
//
// The same launch gives |d|_2 over the REAL state_dict elements of the trainable entries (padding and gaps may hold anything and
// are masked by the entry's geometry, as in agg.hip): d is an fp32 value, its square and every sum are fp64; a thread's serial
// sum, xor-shuffles over the wave, (w0 + w1) + (w2 + w3) through LDS, one partial per chunk; the second stage is one block that
// adds the partials in a fixed order, takes one sqrt and writes a double.  No atomics: the same operands give the same 8 bytes.
// Like the optimizer kernels both stages take the engine's skip word and never synchronise with the host.
#include "common.h"
#include "kernels.h"
#include "../../include/fedmlp_hip_server.h"

template <int RULE>
struct ServerRule {
    ServerOps a;
    bool x_quad;              // the caller's x is 16-byte aligned
    struct Hp {};             // the scalars travel with the operands
    struct Quad { f32x4 x, a, m, v, d; };
    __device__ __forceinline__ void load(Quad& q, int64_t o) const
    {
        if (x_quad) {
            q.x = *reinterpret_cast<const f32x4*>(a.x + o);
        } else {            // a caller's buffer off a 16-byte boundary
#pragma unroll
            for (int k = 0; k < 4; ++k) q.x[k] = a.x[o + k];
        }
        q.a = *reinterpret_cast<const f32x4*>(a.st + o);
        q.m = *reinterpret_cast<const f32x4*>(a.m + o);
        if (RULE != FM_SERVER_AVGM) q.v = *reinterpret_cast<const f32x4*>(a.v + o);
    }
    // q.d = d of the four elements; q.a becomes x'
    __device__ __forceinline__ void update(Quad& q, const Hp&) const
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float x = q.x[k];
            const float d = q.a[k] - x;
            float m = q.m[k];
            if (RULE == FM_SERVER_AVGM) {
                const float t = a.beta1 * m;
                m = t + d;
            } else {
                const float t = a.beta1 * m;
                const float u = a.omb1 * d;
                m = t + u;
            }
            float step;
            if (RULE == FM_SERVER_AVGM) {
                step = a.lr * m;
            } else {
                float v = q.v[k];
                const float sq = d * d;
                if (RULE == FM_SERVER_ADAGRAD) {
                    v = v + sq;
                } else if (RULE == FM_SERVER_ADAM) {
                    const float t = a.beta2 * v;
                    const float u = a.omb2 * sq;
                    v = t + u;
                } else {
                    const float w = v - sq;
                    const float s = w > 0.f ? 1.f : (w < 0.f ? -1.f : 0.f);
                    float u = a.omb2 * sq;
                    u = u * s;
                    v = v - u;
                }
                float r = sqrtf(v);
                r = r + a.tau;
                float t = a.lr * m;
                t = t / r;
                step = t;
                q.v[k] = v;
            }
            q.m[k] = m;
            q.a[k] = x + step;
            q.d[k] = d;
        }
    }
    __device__ __forceinline__ void store(const Quad& q, int64_t o, int64_t begin, int64_t end) const
    {
        store_own(a.st, o, begin, end, q.a);
        store_own(a.m, o, begin, end, q.m);
        if (RULE != FM_SERVER_AVGM) store_own(a.v, o, begin, end, q.v);
    }
};

// sum of d*d in fp64 over the quad's floats that are the chunk's own AND real state_dict elements
__device__ __forceinline__ double srv_sq(const ArenaEntry& en, int64_t o, int64_t begin, int64_t end, const f32x4 d)
{
#pragma clang fp contract(off)
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t g = o + k;
        const bool ok = g >= begin && g < end && real_element(en, g);
        const double e = (double)d[k];
        s = s + (ok ? e * e : 0.0);
    }
    return s;
}

template <int RULE>
__global__ void __launch_bounds__(256) server_opt_kernel(const ServerRule<RULE> r, const ArenaEntry* __restrict__ ent,
                                                         const ArenaChunk* __restrict__ chunks, double* __restrict__ part,
                                                         const int* __restrict__ skip)
{
    if (skip && *skip) return;
    __shared__ double sm[4][1];
    const ArenaChunk ch = chunks[blockIdx.x];
    const ArenaEntry en = ent[ch.ent];
    const int64_t begin = ch.begin, end = begin + ch.len;
    double acc[1] = {0.0};
    arena_walk(r, ch, {}, [&](const typename ServerRule<RULE>::Quad& q, int64_t o) { acc[0] = acc[0] + srv_sq(en, o, begin, end, q.d); });
    const double s = block_sum_f64(acc, 1, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// one block: thread t adds the partials t, t + 256, ... in that order, a fixed halving tree over the 256 sums, one sqrt
__global__ void __launch_bounds__(256) server_norm_final_kernel(const double* __restrict__ part, int nparts, double* __restrict__ norm,
                                                                const int* __restrict__ skip)
{
    if (skip && *skip) return;
    __shared__ double sm[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) s = s + part[i];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] = sm[threadIdx.x] + sm[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *norm = sqrt(sm[0]);
}

template <int RULE>
static void server_launch(const ServerOps& a, const ArenaEntry* ent, const ArenaChunk* chunks, int n_chunks, double* part, hipStream_t s,
                          const int* skip)
{
    const ServerRule<RULE> r{a, (reinterpret_cast<uintptr_t>(a.x) & 15) == 0};
    hipLaunchKernelGGL((server_opt_kernel<RULE>), dim3(n_chunks), dim3(256), 0, s, r, ent, chunks, part, skip);
}

void k_server_opt(int rule, const ServerOps& a, const ArenaEntry* ent, const ArenaChunk* chunks, int n_chunks, double* part,
                  double* norm, hipStream_t s, const int* skip)
{
    if (n_chunks <= 0) return;
    switch (rule) {
    case FM_SERVER_AVGM: server_launch<FM_SERVER_AVGM>(a, ent, chunks, n_chunks, part, s, skip); break;
    case FM_SERVER_ADAGRAD: server_launch<FM_SERVER_ADAGRAD>(a, ent, chunks, n_chunks, part, s, skip); break;
    case FM_SERVER_ADAM: server_launch<FM_SERVER_ADAM>(a, ent, chunks, n_chunks, part, s, skip); break;
    default: server_launch<FM_SERVER_YOGI>(a, ent, chunks, n_chunks, part, s, skip); break;
    }
    if (norm) hipLaunchKernelGGL(server_norm_final_kernel, dim3(1), dim3(256), 0, s, part, n_chunks, norm, skip);
}

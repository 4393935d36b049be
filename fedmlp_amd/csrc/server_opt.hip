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
// Grid: one block of 256 threads per chunk of <= FM_DIST_CHUNK floats of ONE trainable state entry (agg.hip's DistEntry /
// DistChunk geometry, restricted by the engine to the entries inside the parameter arena).  An entry begins and ends at any
// element offset: a chunk's first quad starts at the 16-byte boundary at or below its begin, a block reads whole quads and
// WRITES only its own floats (optim.hip's rule).  Padding inside an entry's span (a == x == 0) is stepped like any element and
// stays an exact zero: d = 0, m = 0, t = 0 (r >= tau > 0).  Floats outside every span are touched by nobody.
//
// The same launch gives |d|_2 over the REAL state_dict elements of the trainable entries (padding and gaps may hold anything and
// are masked by the entry's geometry, as in agg.hip): d is an fp32 value, its square and every sum are fp64; a thread's serial
// sum, xor-shuffles over the wave, (w0 + w1) + (w2 + w3) through LDS, one partial per chunk; the second stage is one block that
// adds the partials in a fixed order, takes one sqrt and writes a double.  No atomics: the same operands give the same 8 bytes.
// Like the optimizer kernels both stages take the engine's skip word and never synchronise with the host.
#include "common.h"
#include "kernels.h"
#include "../../include/fedmlp_hip_server.h"

// a thread holds SRV_QPT quads of every operand: all its 16-byte loads are in flight before the first use
#define SRV_QPT (FM_DIST_CHUNK / 4 / 256)

template <int RULE>
struct ServerRule {
    ServerOps a;
    struct Quad { f32x4 x, a, m, v; };
    __device__ __forceinline__ void load(Quad& q, int64_t o, bool x_quad) const
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
    // -> d of the four elements; q.a becomes x'
    __device__ __forceinline__ f32x4 update(Quad& q) const
    {
#pragma clang fp contract(off)
        f32x4 dd;
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
            dd[k] = d;
        }
        return dd;
    }
};

// the floats of the quad at o that lie in [begin, end): 16 bytes inside, lane by lane at an entry's edges
__device__ __forceinline__ void srv_store_own(float* __restrict__ a, int64_t o, int64_t begin, int64_t end, const f32x4 v)
{
    if (o >= begin && o + 4 <= end) {
        *reinterpret_cast<f32x4*>(a + o) = v;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (o + k >= begin && o + k < end) a[o + k] = v[k];
    }
}

// sum of d*d in fp64 over the quad's floats that are the chunk's own AND real state_dict elements (agg.hip's test)
__device__ __forceinline__ double srv_sq(const DistEntry& en, int64_t o, int64_t begin, int64_t end, const f32x4 d)
{
#pragma clang fp contract(off)
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t g = o + k;
        bool ok = g >= begin && g < end;
        if (!en.all_real) {
            const unsigned pos = (unsigned)(g - en.off) % (unsigned)en.row;      // inside the row of one output channel
            const unsigned ip = pos % (unsigned)en.Ipad, wp = (pos / (unsigned)en.Ipad) % (unsigned)en.Wpad;
            ok = ok && pos < (unsigned)en.dense && ip < (unsigned)en.I && wp < (unsigned)en.W;
        }
        const double e = (double)d[k];
        s = s + (ok ? e * e : 0.0);
    }
    return s;
}

template <int RULE>
__global__ void __launch_bounds__(256) server_opt_kernel(const ServerRule<RULE> r, const DistEntry* __restrict__ ent,
                                                         const DistChunk* __restrict__ chunks, int x_quad,
                                                         double* __restrict__ part, const int* __restrict__ skip)
{
    if (skip && *skip) return;
    __shared__ double sm[4];
    const DistChunk ch = chunks[blockIdx.x];
    const DistEntry en = ent[ch.entry];
    const int64_t begin = en.off + ch.start;
    const int64_t end = en.off + min(ch.start + FM_DIST_CHUNK, en.len);
    const int64_t o0 = (begin & ~(int64_t)3) + 4 * (int64_t)threadIdx.x;
    double acc = 0.0;
    typename ServerRule<RULE>::Quad q[SRV_QPT];
#pragma unroll
    for (int j = 0; j < SRV_QPT; ++j) {
        const int64_t o = o0 + (int64_t)j * 1024;
        if (o < end) r.load(q[j], o, x_quad != 0);
    }
#pragma unroll
    for (int j = 0; j < SRV_QPT; ++j) {
        const int64_t o = o0 + (int64_t)j * 1024;
        if (o < end) {
            const f32x4 d = r.update(q[j]);
            srv_store_own(r.a.st, o, begin, end, q[j].a);
            srv_store_own(r.a.m, o, begin, end, q[j].m);
            if (RULE != FM_SERVER_AVGM) srv_store_own(r.a.v, o, begin, end, q[j].v);
            acc = acc + srv_sq(en, o, begin, end, d);
        }
    }
    // a full chunk that starts off a 16-byte boundary has one quad more than SRV_QPT * 256
    const int64_t o = o0 + (int64_t)SRV_QPT * 1024;
    if (o < end) {
        typename ServerRule<RULE>::Quad t;
        r.load(t, o, x_quad != 0);
        const f32x4 d = r.update(t);
        srv_store_own(r.a.st, o, begin, end, t.a);
        srv_store_own(r.a.m, o, begin, end, t.m);
        if (RULE != FM_SERVER_AVGM) srv_store_own(r.a.v, o, begin, end, t.v);
        acc = acc + srv_sq(en, o, begin, end, d);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) acc = acc + __shfl_xor(acc, s, 64);
    if (lane == 0) sm[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
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
static void server_launch(const ServerOps& a, const DistEntry* ent, const DistChunk* chunks, int n_chunks, double* part, hipStream_t s,
                          const int* skip)
{
    const ServerRule<RULE> r{a};
    const int x_quad = (reinterpret_cast<uintptr_t>(a.x) & 15) == 0 ? 1 : 0;
    hipLaunchKernelGGL((server_opt_kernel<RULE>), dim3(n_chunks), dim3(256), 0, s, r, ent, chunks, x_quad, part, skip);
}

void k_server_opt(int rule, const ServerOps& a, const DistEntry* ent, const DistChunk* chunks, int n_chunks, double* part,
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

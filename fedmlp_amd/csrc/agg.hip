// RSCFed aggregation (utils/FedAvg.py:16-49): the per-entry distances behind model_dist.
//
// fm_state_dist: for K engine-layout client states and a reference state (given, or their unweighted Fed_w mean formed in
// registers with the fold's roundings: ((s0 + s1) + ...) / float(K), never written to HBM), the fp32 L2 norm of
// (state_k - ref) over every fp32 state_dict entry, norms[K][n_entries] in state_dict order.  HBM-bound: every state is read
// once, (K [+ 1]) x 4 B per arena element, 16 B per lane.
//
// The engine layout is not the state_dict layout: a conv weight is [O][KH][Wpad][Ipad] with a row stride that may exceed the
// dense row (packed stem), and only wp < KW, ip < I are state_dict elements.  Padding inside a matrix is zero after
// fm_set_state but nothing here relies on it, and the gaps outside the matrices hold whatever the caller left there: an
// element counts only if the entry's geometry says it is real.  The kernel is driven by the engine's entry / chunk table
// (arena_table.h): one block per chunk, all of them.
//
// Precision and determinism: the difference in fp32 (what torch.norm(w1 - w2) sees), its square and every sum in fp64.  No
// atomics: stage 1 is one block per chunk, a thread's serial sum, xor-shuffles over the wave and (w0 + w1) + (w2 + w3) through
// LDS, one fp64 partial per (chunk, k); stage 2 is one thread per (entry, k) adding the entry's partials in chunk order, then
// sqrt and one rounding to fp32.  The fp64 sum of n <= 2^22 squares is off by < n 2^-53 relative, so each norm is the
// correctly rounded norm of the fp32 differences to within one fp32 ulp, whatever the chunking.
#include "kernels.h"

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// four consecutive arena floats from g4 (a multiple of 4): one 16-byte load where the pointer is 16-byte aligned and the
// quad lies inside the arena, else element by element (elements outside the arena read as zero and are never counted)
__device__ __forceinline__ void dist_load4(const float* __restrict__ p, int64_t g4, bool quad, int64_t NS, float (&v)[4])
{
    if (quad) {
        const float4 t = *reinterpret_cast<const float4*>(p + g4);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = (g4 + c < NS) ? p[g4 + c] : 0.f;
    }
}

template <int KMAX>
__global__ void __launch_bounds__(256) state_dist_kernel(FoldArgs a, int K, const float* __restrict__ ref,
                                                         const ArenaEntry* __restrict__ ent, const ArenaChunk* __restrict__ chunks,
                                                         int64_t NS, int aligned, double* __restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ double sm[4][KMAX];
    const ArenaChunk ch = chunks[blockIdx.x];
    const ArenaEntry en = ent[ch.ent];
    const int64_t begin = ch.begin, end = begin + ch.len;
    const float Kf = (float)K;
    double acc[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) acc[k] = 0.0;
    // the chunk's first quad starts at the 16-byte boundary at or below `begin` (an entry may start at any element offset):
    // its leading elements belong to the neighbour and are masked like the trailing ones of the last quad
    for (int64_t g4 = (begin & ~(int64_t)3) + 4 * (int64_t)threadIdx.x; g4 < end; g4 += 4 * 256) {
        const bool quad = aligned && g4 + 4 <= NS;
        float v[KMAX][4], r[4];
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) dist_load4(a.s[k], g4, quad, NS, v[k]);
        if (ref) {
            dist_load4(ref, g4, quad, NS, r);
        } else {            // Fed_w(states, [1]*K): products with 1.0f are exact, sums left to right, one IEEE division
#pragma unroll
            for (int c = 0; c < 4; ++c) r[c] = v[0][c];
#pragma unroll
            for (int k = 1; k < KMAX; ++k)
                if (k < K) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) r[c] = r[c] + v[k][c];
                }
#pragma unroll
            for (int c = 0; c < 4; ++c) r[c] = r[c] / Kf;
        }
        bool ok[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t g = g4 + c;
            ok[c] = g >= begin && g < end && real_element(en, g);
        }
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const double d = (double)(v[k][c] - r[c]);       // the difference is an fp32 value
                    acc[k] = acc[k] + (ok[c] ? d * d : 0.0);
                }
            }
    }
    const double s = block_sum_f64(acc, K, sm);
    if ((int)threadIdx.x < K) part[(int64_t)blockIdx.x * K + threadIdx.x] = s;
}

// one thread per (entry, k), k fastest: the entry's partials in chunk order, square root, one rounding to fp32
__global__ void __launch_bounds__(64) state_dist_final_kernel(const double* __restrict__ part, const ArenaEntry* __restrict__ ent,
                                                              int n_entries, int K, float* __restrict__ norms)
{
    const int idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= n_entries * K) return;
    const int e = idx / K, k = idx % K;
    const double* p = part + (int64_t)ent[e].chunk0 * K + k;
    const int n = ent[e].nchunks;
    double s = 0.0;
#pragma unroll 8
    for (int j = 0; j < n; ++j) s = s + p[(int64_t)j * K];
    norms[(int64_t)k * n_entries + e] = (float)sqrt(s);
}

void k_state_dist(const FoldArgs& a, int K, const float* ref, const ArenaEntry* ent, int n_entries, const ArenaChunk* chunks,
                  int n_chunks, int64_t NS, double* part, float* norms, hipStream_t s)
{
    bool al = ref == nullptr || (reinterpret_cast<uintptr_t>(ref) & 15) == 0;
    for (int k = 0; k < K; ++k) al = al && (reinterpret_cast<uintptr_t>(a.s[k]) & 15) == 0;
    if (K <= 8)
        hipLaunchKernelGGL(state_dist_kernel<8>, dim3(n_chunks), dim3(256), 0, s, a, K, ref, ent, chunks, NS, al ? 1 : 0, part);
    else
        hipLaunchKernelGGL(state_dist_kernel<FM_FOLD_MAX>, dim3(n_chunks), dim3(256), 0, s, a, K, ref, ent, chunks, NS, al ? 1 : 0,
                           part);
    hipLaunchKernelGGL(state_dist_final_kernel, dim3(cdiv(n_entries * K, 64)), dim3(64), 0, s, part, ent, n_entries, K, norms);
}

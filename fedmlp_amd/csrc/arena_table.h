// The entry / chunk table of the state arena, and everything a kernel needs to walk it "one block of 256 threads per chunk of
// at most FM_DIST_CHUNK floats of ONE state entry": the model distance (agg.hip), the grouped / masked optimizer steps and the
// masked accumulate (optim.hip), the masked client-drift correction (drift.hip) and the server optimizers (server_opt.hip).
// One table per engine, built once from its state entries by arena_table_build (plain host C++: tests/host/ compiles it alone).
//
// The contract every kernel's bits rest on:
//  1. Chunk geometry.  Every fp32 entry's span [off, off + len) is cut at multiples of FM_DIST_CHUNK counted from `off`: a
//     chunk never straddles an entry.  A conv weight's span is its O rows with the row stride (the packed stem's row tails
//     included), a vector's span its n elements; int64 counters get no entry.
//  2. Chunk order.  The chunks of the PARAMETER entries come first, [0, n_param_chunks), then those of the buffer entries (the
//     running statistics); each class in state_dict order, an entry's chunks in ascending start.  A kernel over the
//     parameters launches the prefix, and a sum over its partials in block order is a sum in that order; a per-entry sum goes
//     through chunk0 / nchunks and does not see how entries are ordered against each other.
//     `ent` -- ArenaChunk::ent, the selector's index, fm_state_dist's output column -- counts the fp32 entries in state_dict
//     order, parameters and buffers alike.
//  3. Per-thread work (arena_walk).  A chunk's first quad sits at the 16-byte boundary at or below `begin`; thread t takes quads
//     t, t + 256, ...; all ARENA_QPT loads are issued before the first use; a full chunk that starts off a 16-byte boundary
//     has one quad more (the 2049th), which thread 0 takes after the others.  A block reads whole quads -- the neighbour's
//     lanes are computed and dropped -- and WRITES only its own floats (store_own), so floats outside every entry are touched by
//     nobody and padding inside a span is stepped with its entry.
//  4. Arithmetic.  A rule's update() and every fp64 sum here are written under `fp contract(off)` in a fixed order.
#pragma once
#include <algorithm>
#include <vector>

#define FM_DIST_CHUNK 8192
#define OPT_MAX_ENT 512

// one fp32 state entry: the arena span [off, off + len), rows of `row` floats of which the first `dense` are [..][Wpad][Ipad]
// with wp < W, ip < I real state_dict elements (all_real: every element of the span is); its chunks are chunk0 .. chunk0 +
// nchunks - 1
struct ArenaEntry { long long off; int len, row, dense, Ipad, I, Wpad, W, chunk0, nchunks, all_real; };
// <= FM_DIST_CHUNK consecutive arena floats of entry `ent`: a block finds its floats without a dependent load
struct ArenaChunk { long long begin; int len; int ent; };
// four bits per entry, by value with the launch (no device table to keep in step).  The grouped steps: the entry's parameter
// group, or OPT_SKIP = nobody steps it (no group, or frozen).  The masked passes: 0 = trainable, anything else = frozen.  A
// buffer entry's nibble is never read: no selector kernel launches its chunks.
struct OptSel { unsigned w[OPT_MAX_ENT / 8]; };
static inline void opt_sel_set(OptSel& t, int ent, unsigned v) { t.w[ent >> 3] = (t.w[ent >> 3] & ~(15u << ((ent & 7) * 4))) | (v << ((ent & 7) * 4)); }

// ---- the builder ---------------------------------------------------------------------------------------------------
struct ArenaSpan { int dense, row; long long len; };
// one state_dict entry as the builder sees it.  kind 0: a weight, rows of [..][Wpad][Ipad] with W x I real; 1: a float vector;
// 2: an int64 counter (no table entry).  param: the entry lies in the trainable arena [0, NP)
struct ArenaDesc { int kind; long long off; ArenaSpan span; int Ipad, I, Wpad, W; bool param; };
struct ArenaTableHost {
    std::vector<ArenaEntry> ent;        // the fp32 entries in state_dict order
    std::vector<ArenaChunk> chunks;     // parameter chunks, then buffer chunks
    std::vector<int> ent_of;            // descriptor -> its index in `ent`, -1 for a counter
    int n_param_chunks = 0;
};
// -> null, or why the list is refused
inline const char* arena_table_build(const std::vector<ArenaDesc>& descs, long long NP, long long NS, ArenaTableHost& t)
{
    t = ArenaTableHost{};
    for (const ArenaDesc& d : descs) {
        if (d.kind == 2) { t.ent_of.push_back(-1); continue; }
        ArenaEntry a{};
        a.off = d.off; a.len = (int)d.span.len; a.row = d.span.row; a.dense = d.span.dense;
        if (d.kind == 0) { a.Ipad = d.Ipad; a.I = d.I; a.Wpad = d.Wpad; a.W = d.W; }
        else a.Ipad = a.I = a.Wpad = a.W = 1;
        a.all_real = a.row == a.dense && a.Ipad == a.I && a.Wpad == a.W;
        if (d.param && (d.span.len <= 0 || d.off < 0 || d.off + d.span.len > NP)) return "a parameter entry lies outside the trainable arena";
        if (d.span.len <= 0 || d.off < 0 || d.off + d.span.len > NS) return "state entry outside the arena";
        t.ent_of.push_back((int)t.ent.size());
        t.ent.push_back(a);
    }
    if (t.ent.size() > OPT_MAX_ENT) return "more parameter entries than the optimizer table holds";
    for (int params = 1; params >= 0; --params) {
        for (size_t i = 0; i < descs.size(); ++i) {
            if (t.ent_of[i] < 0 || (int)descs[i].param != params) continue;
            ArenaEntry& a = t.ent[t.ent_of[i]];
            a.chunk0 = (int)t.chunks.size();
            for (int st = 0; st < a.len; st += FM_DIST_CHUNK) t.chunks.push_back({a.off + st, std::min(FM_DIST_CHUNK, a.len - st), t.ent_of[i]});
            a.nchunks = (int)t.chunks.size() - a.chunk0;
        }
        if (params) t.n_param_chunks = (int)t.chunks.size();
    }
    return nullptr;
}

// ---- the device side -------------------------------------------------------------------------------------------------
#ifdef __HIPCC__
#include "common.h"

// a thread holds ARENA_QPT quads of every operand
#define ARENA_QPT (FM_DIST_CHUNK / 4 / 256)

__device__ __forceinline__ unsigned opt_sel_get(const OptSel& t, int ent) { return (t.w[ent >> 3] >> ((ent & 7) * 4)) & 15u; }

// the floats of the quad at o that lie in [begin, end): 16 bytes inside, lane by lane at an entry's edges
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

// is arena float g of entry `en` a real state_dict element (padding and row tails may hold anything and are never counted)
__device__ __forceinline__ bool real_element(const ArenaEntry& en, int64_t g)
{
    if (en.all_real) return true;
    const unsigned pos = (unsigned)(g - en.off) % (unsigned)en.row;      // inside the row of one output channel
    const unsigned ip = pos % (unsigned)en.Ipad, wp = (pos / (unsigned)en.Ipad) % (unsigned)en.Wpad;
    return pos < (unsigned)en.dense && ip < (unsigned)en.I && wp < (unsigned)en.W;
}

// The fixed-order fp64 sum of a block of 256 threads, for the first n of N values per thread: xor-shuffles over the wave, then
// the four waves through LDS as (w0 + w1) + (w2 + w3).  Thread k < n returns the sum of acc[k]; one barrier, which every
// thread of the block must reach.
template <int N>
__device__ __forceinline__ double block_sum_f64(const double (&acc)[N], int n, double (&sm)[4][N])
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k)
        if (k < n) {
            double s = acc[k];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) s = s + __shfl_xor(s, o, 64);
            if (lane == 0) sm[wave][k] = s;
        }
    __syncthreads();
    const int k = threadIdx.x;
    return k < n ? (sm[0][k] + sm[1][k]) + (sm[2][k] + sm[3][k]) : 0.0;
}

// The chunk walker (contract 3) over a rule R: r.load(Quad&, o) reads a quad of every operand at float offset o (a multiple of
// 4), R::update / r.update(Quad&, hp) holds the arithmetic, r.store(Quad, o, begin, end) writes the quad's floats inside
// [begin, end).  after(q, o) runs behind each quad's store (the server optimizers' sum of squares).
template <class R, class F>
__device__ __forceinline__ void arena_walk(const R& r, const ArenaChunk ch, const typename R::Hp& hp, F&& after)
{
    const int64_t begin = ch.begin, end = begin + ch.len;
    const int64_t o0 = (begin & ~(int64_t)3) + 4 * (int64_t)threadIdx.x;
    typename R::Quad q[ARENA_QPT];
#pragma unroll
    for (int j = 0; j < ARENA_QPT; ++j) {
        const int64_t o = o0 + (int64_t)j * 1024;
        if (o < end) r.load(q[j], o);
    }
#pragma unroll
    for (int j = 0; j < ARENA_QPT; ++j) {
        const int64_t o = o0 + (int64_t)j * 1024;
        if (o < end) {
            r.update(q[j], hp);
            r.store(q[j], o, begin, end);
            after(q[j], o);
        }
    }
    const int64_t o = o0 + (int64_t)ARENA_QPT * 1024;
    if (o < end) {
        typename R::Quad t;
        r.load(t, o);
        r.update(t, hp);
        r.store(t, o, begin, end);
        after(t, o);
    }
}
template <class R>
__device__ __forceinline__ void arena_walk(const R& r, const ArenaChunk ch, const typename R::Hp& hp)
{
    arena_walk(r, ch, hp, [](const typename R::Quad&, int64_t) {});
}
#endif

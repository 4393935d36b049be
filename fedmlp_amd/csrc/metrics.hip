// globaltest's metrics on the device (utils/evaluations.py:41-66, utils/multilabel_metrixs.py): per class the four
// threshold counts {tp, npos, npred, tn}, sklearn's average precision and the area under the ROC curve, with every tie
// grouped, from fp32 [N][C] scores and labels.  No sort: for a positive sample i
//   ge_pos(i) = #{j positive : s_j >= s_i}     lt_neg(i) = #{j negative : s_j < s_i}     eq_neg(i) = #{j negative : s_j == s_i}
//   ge_all(i) = ge_pos(i) + (Nn - lt_neg(i))   (no NaN scores: every negative is either < or >=)
//   AP = (sum_i (double)ge_pos / (double)ge_all) / P          AUC = (double)(sum_i 2 lt_neg + eq_neg) / (2.0 P Nn)
// The compares are IEEE fp32 compares on the scores as given (-0.0 == +0.0).
//
// Passes, all on one stream, no atomics:
//   count    one wave per FM_METRICS_ROWS rows: ballots -> the four counts of every (class, chunk)
//   scan     one block per class: exclusive scan of the chunks' positives (where each chunk's positives go), the class's totals
//   scatter  the count pass again with the offsets: class-major scores sT[c] = [positives in row order | negatives in row order],
//            so the pair pass needs no label bits: the first P scores of a class are its positives
//   pair     grid (tiles of FM_METRICS_BP positives, C): a thread owns one positive and three integer counters; the class's
//            scores stream through LDS in tiles of FM_METRICS_TILE, every lane reading the same 16 bytes (a broadcast, no bank
//            conflicts).  Per block a fixed-order reduction (xor-shuffles over the wave, (w0 + w1) + (w2 + w3) through LDS): one fp64
//            and one int64 partial
//   final    one thread per class adds the partials in block order
// Every count is an exact integer, so only the fp64 sum of the AP terms has an order, and that order is fixed: two calls give the
// same bits.  The AUC numerator is < 2 N^2 <= 2^45 and its denominator 2 P Nn <= 2^44: both exact in fp64, one rounding.
// Work: P N compares for the positives' segment plus 2 P Nn for the negatives'; a 5-15 % prevalence test set does a tenth of N^2.
#include "kernels.h"

namespace {

struct MetricsWs {
    float* sT;            // [C][N]
    int4* chunk_cnt;      // [C][nchunks] {tp, npos, npred, tn} of a chunk
    int* pos_off;         // [C][nchunks] positives of the class before the chunk
    long long* tot;       // [C][4]
    double* part_ap;      // [C][ntiles]
    long long* part_auc;  // [C][ntiles]
};

inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

MetricsWs carve(void* ws, int64_t N, int C)
{
    const size_t nch = (size_t)cdiv64(N, FM_METRICS_ROWS), nt = (size_t)cdiv64(N, FM_METRICS_BP);
    char* p = static_cast<char*>(ws);
    MetricsWs w;
    w.sT = reinterpret_cast<float*>(p);            p += up16((size_t)C * N * 4);
    w.chunk_cnt = reinterpret_cast<int4*>(p);      p += up16((size_t)C * nch * 16);
    w.pos_off = reinterpret_cast<int*>(p);         p += up16((size_t)C * nch * 4);
    w.tot = reinterpret_cast<long long*>(p);       p += up16((size_t)C * 4 * 8);
    w.part_ap = reinterpret_cast<double*>(p);      p += up16((size_t)C * nt * 8);
    w.part_auc = reinterpret_cast<long long*>(p);
    return w;
}

// one wave per chunk of 64 rows, a lane per row; SCATTER = false: the chunk's counts, true: the class-major scores
template <bool SCATTER>
__global__ void __launch_bounds__(256) metrics_rows_kernel(const float* __restrict__ scores, const float* __restrict__ labels, int N,
                                                           int C, int nchunks, float thr, int4* __restrict__ chunk_cnt,
                                                           const int* __restrict__ pos_off, const long long* __restrict__ tot,
                                                           float* __restrict__ sT)
{
    const int lane = threadIdx.x & 63;
    const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= nchunks) return;                         // a whole wave leaves: the ballots below see full chunks' lanes only
    const int row = chunk * FM_METRICS_ROWS + lane;
    const bool in = row < N;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int c = 0; c < C; ++c) {
        const float s = in ? scores[(int64_t)row * C + c] : 0.f;
        const bool pos = in && labels[(int64_t)row * C + c] != 0.f;
        const unsigned long long bpos = __ballot(pos);
        if (!SCATTER) {
            const bool pred = in && s > thr;
            const unsigned long long bpred = __ballot(pred), bin = __ballot(in);
            if (lane == 0)
                chunk_cnt[(int64_t)c * nchunks + chunk] =
                    make_int4(__popcll(bpos & bpred), __popcll(bpos), __popcll(bpred), __popcll(bin & ~(bpos | bpred)));
        } else if (in) {
            const int before = pos_off[(int64_t)c * nchunks + chunk];     // positives of earlier chunks
            const int rank = __popcll(bpos & below);                      // positives of this chunk before this row
            // negatives start at P; those before this row: (rows before) - (positives before)
            const int dst = pos ? before + rank : (int)tot[c * 4 + 1] + (chunk * FM_METRICS_ROWS - before) + (lane - rank);
            sT[(int64_t)c * N + dst] = s;
        }
    }
}

// one block per class: thread t owns the chunks [t per, (t + 1) per); the exclusive scan of their positives and the totals
__global__ void __launch_bounds__(256) metrics_scan_kernel(const int4* __restrict__ chunk_cnt, int nchunks, int* __restrict__ pos_off,
                                                           long long* __restrict__ tot, long long* __restrict__ counts)
{
    __shared__ long long sm[256][4];
    __shared__ long long base[256];
    const int c = blockIdx.x, t = threadIdx.x;
    const int per = (nchunks + 255) / 256;
    const int lo = min(t * per, nchunks), hi = min(lo + per, nchunks);
    const int4* cc = chunk_cnt + (int64_t)c * nchunks;
    long long a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    for (int j = lo; j < hi; ++j) {
        const int4 v = cc[j];
        a0 += v.x; a1 += v.y; a2 += v.z; a3 += v.w;
    }
    sm[t][0] = a0; sm[t][1] = a1; sm[t][2] = a2; sm[t][3] = a3;
    __syncthreads();
    if (t < 4) {                                          // integer sums: any order gives the same value
        long long s = 0;
        for (int j = 0; j < 256; ++j) {
            if (t == 1) base[j] = s;
            s += sm[j][t];
        }
        tot[c * 4 + t] = s;
        if (counts) counts[c * 4 + t] = s;
    }
    __syncthreads();
    int run = (int)base[t];
    for (int j = lo; j < hi; ++j) {
        pos_off[(int64_t)c * nchunks + j] = run;
        run += cc[j].y;
    }
}

__global__ void __launch_bounds__(FM_METRICS_BP) metrics_pair_kernel(const float* __restrict__ sT, const long long* __restrict__ tot,
                                                                     int N, int ntiles, double* __restrict__ part_ap,
                                                                     long long* __restrict__ part_auc)
{
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float tile[FM_METRICS_TILE];
    __shared__ double sm_ap[FM_METRICS_BP / 64];
    __shared__ long long sm_auc[FM_METRICS_BP / 64];
    const int c = blockIdx.y, t = threadIdx.x;
    const int P = (int)tot[c * 4 + 1];
    const int i0 = blockIdx.x * FM_METRICS_BP;
    if (i0 >= P) return;                                  // block-uniform: the final pass reads cdiv(P, BP) partials only
    const float* s = sT + (int64_t)c * N;
    const bool live = i0 + t < P;
    const float si = live ? s[i0 + t] : 0.f;
    int ge_pos = 0, lt_neg = 0, eq_neg = 0;
    // the positives' segment [0, P): one compare per pair
    for (int j0 = 0; j0 < P; j0 += FM_METRICS_TILE) {
        const int cnt = min(FM_METRICS_TILE, P - j0);
        __syncthreads();
        for (int k = t; k < cnt; k += FM_METRICS_BP) tile[k] = s[j0 + k];
        __syncthreads();
        int k = 0;
        for (; k + 4 <= cnt; k += 4) {
            const float4 v = *reinterpret_cast<const float4*>(tile + k);
            ge_pos += (v.x >= si) + (v.y >= si) + (v.z >= si) + (v.w >= si);
        }
        for (; k < cnt; ++k) ge_pos += tile[k] >= si;
    }
    // the negatives' segment [P, N): strictly below, and equal
    for (int j0 = P; j0 < N; j0 += FM_METRICS_TILE) {
        const int cnt = min(FM_METRICS_TILE, N - j0);
        __syncthreads();
        for (int k = t; k < cnt; k += FM_METRICS_BP) tile[k] = s[j0 + k];
        __syncthreads();
        int k = 0;
        for (; k + 4 <= cnt; k += 4) {
            const float4 v = *reinterpret_cast<const float4*>(tile + k);
            lt_neg += (v.x < si) + (v.y < si) + (v.z < si) + (v.w < si);
            eq_neg += (v.x == si) + (v.y == si) + (v.z == si) + (v.w == si);
        }
        for (; k < cnt; ++k) {
            lt_neg += tile[k] < si;
            eq_neg += tile[k] == si;
        }
    }
    const int ge_all = ge_pos + ((N - P) - lt_neg);
    double ap = live ? (double)ge_pos / (double)ge_all : 0.0;     // a live positive counts itself: ge_all >= ge_pos >= 1
    long long au = live ? 2ll * lt_neg + eq_neg : 0ll;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        ap = ap + __shfl_xor(ap, o, 64);
        au = au + __shfl_xor(au, o, 64);
    }
    if ((t & 63) == 0) { sm_ap[t >> 6] = ap; sm_auc[t >> 6] = au; }
    __syncthreads();
    if (t == 0) {
        part_ap[(int64_t)c * ntiles + blockIdx.x] = (sm_ap[0] + sm_ap[1]) + (sm_ap[2] + sm_ap[3]);
        part_auc[(int64_t)c * ntiles + blockIdx.x] = (sm_auc[0] + sm_auc[1]) + (sm_auc[2] + sm_auc[3]);
    }
}

// one thread per class: the partials in block order
__global__ void __launch_bounds__(64) metrics_final_kernel(const double* __restrict__ part_ap, const long long* __restrict__ part_auc,
                                                           const long long* __restrict__ tot, int N, int C, int ntiles,
                                                           double* __restrict__ ap, double* __restrict__ auc)
{
#pragma clang fp contract(off)
    const int c = threadIdx.x;
    if (c >= C) return;
    const long long P = tot[c * 4 + 1], Nn = (long long)N - P;
    const int n = (int)((P + FM_METRICS_BP - 1) / FM_METRICS_BP);
    double sa = 0.0;
    long long su = 0;
    for (int j = 0; j < n; ++j) {
        sa = sa + part_ap[(int64_t)c * ntiles + j];
        su += part_auc[(int64_t)c * ntiles + j];
    }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (ap) ap[c] = P > 0 ? sa / (double)P : nan;
    if (auc) auc[c] = (P > 0 && Nn > 0) ? (double)su / (2.0 * (double)P * (double)Nn) : nan;
}

}  // namespace

size_t fm_metrics_ws_bytes(int64_t N, int C)
{
    const size_t nch = (size_t)cdiv64(N, FM_METRICS_ROWS), nt = (size_t)cdiv64(N, FM_METRICS_BP);
    return up16((size_t)C * N * 4) + up16((size_t)C * nch * 16) + up16((size_t)C * nch * 4) + up16((size_t)C * 4 * 8) +
           2 * up16((size_t)C * nt * 8);
}

void k_eval_metrics(const float* scores, const float* labels, int64_t N, int C, float threshold, void* ws, double* ap, double* auc,
                    int64_t* counts, hipStream_t s)
{
    const MetricsWs w = carve(ws, N, C);
    const int n = (int)N, nch = (int)cdiv64(N, FM_METRICS_ROWS), nt = (int)cdiv64(N, FM_METRICS_BP);
    const dim3 rows_grid((unsigned)cdiv64(nch, 4));
    hipLaunchKernelGGL(metrics_rows_kernel<false>, rows_grid, dim3(256), 0, s, scores, labels, n, C, nch, threshold, w.chunk_cnt,
                       (const int*)nullptr, (const long long*)nullptr, (float*)nullptr);
    hipLaunchKernelGGL(metrics_scan_kernel, dim3(C), dim3(256), 0, s, w.chunk_cnt, nch, w.pos_off, w.tot,
                       reinterpret_cast<long long*>(counts));
    if (!ap && !auc) return;
    hipLaunchKernelGGL(metrics_rows_kernel<true>, rows_grid, dim3(256), 0, s, scores, labels, n, C, nch, threshold, (int4*)nullptr,
                       w.pos_off, w.tot, w.sT);
    hipLaunchKernelGGL(metrics_pair_kernel, dim3(nt, C), dim3(FM_METRICS_BP), 0, s, w.sT, w.tot, n, nt, w.part_ap, w.part_auc);
    hipLaunchKernelGGL(metrics_final_kernel, dim3(1), dim3(64), 0, s, w.part_ap, w.part_auc, w.tot, n, C, nt, ap, auc);
}

// Classifier head, loss heads, prototype pass, cosine tagging, top-k selection.
// gfx950; every kernel here is small (B x C or N x D work) and latency/HBM bound.
//
// Reference arithmetic restated (utils/local_training.py unless noted):
//   adaptive_avg_pool2d(1)+flatten -> feature, nn.Linear -> logits   (:657 via model)
//   nn.BCEWithLogitsLoss(pos_weight, 'none').sum()/(bs*C)             (:642, 664-665)
//   stage-1 BCE-on-probabilities(active) + MSE-to-teacher(missing)    (:937-963, FedNoRo.py:22)
//   stage-2 masked BCE-on-probabilities                               (:1183-1188)
//   FixMatch weak/strong loss                                         (:797-815)
//   FedLSR mixed-prediction BCE + beta JS, two views                  (:1258-1269, 1294-1314)
//   FedIRM supervised / relation-phase heads, relation matrices       (:73-113, 370-376, 421-452)
//   RSCFed BCE(active) + probability MSE to the EMA teacher           (:719, 740-743)
//   FedNoRo LA_KD: BCE-on-probabilities + MSE to sigmoid(teacher/0.8) (utils/FedNoRo.py:35-38, :143-151)
//   CBAFed warm-up / stage-2 pseudo-labels, loss_w and counts         (:247-269, 303-333)
//   RoFL small-loss selection, centroid vote, RFLloss, centroid blend (:524-572, 582-626)
//   prototype masked sums + confident-count t                         (:985-994, 1229-1238)
//   CosineSimilarityFast difference                                   (:1417-1435, 1056-1057)
//   stable top-k / bottom-k                                           (utils/utils.py:24-35)
// Loss kernels also emit dloss/dlogits with the exact autograd formulas of the
// torch ops the reference calls (binary_cross_entropy backward divides by
// max(p(1-p), 1e-12); log terms clamp at -100).
#include "common.h"
#include "kernels.h"

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// block-wide deterministic sum (256 threads); result valid in every thread
__device__ __forceinline__ float block_sum(float v, float* sh /*[4]*/)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__device__ __forceinline__ float sigmoidf_(float z) { return 1.f / (1.f + expf(-z)); }

// ------------------------------------------------------------ avgpool / fc -----
template <typename T>
__global__ void avgpool_kernel(const T* __restrict__ x, float* __restrict__ feat, int HW, int C)
{
    const int img = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float s = 0.f;
#pragma unroll 7
        for (int p = 0; p < HW; ++p) s += (float)x[((size_t)img * HW + p) * C + c];
        feat[(size_t)img * C + c] = s / (float)HW;
    }
}
void k_avgpool(const void* x, int dt, float* feat, int imgs, int HW, int C, hipStream_t s)
{
    if (dt == DT_F32)
        hipLaunchKernelGGL(avgpool_kernel<float>, dim3(imgs), dim3(256), 0, s, reinterpret_cast<const float*>(x), feat, HW, C);
    else
        hipLaunchKernelGGL(avgpool_kernel<bf16>, dim3(imgs), dim3(256), 0, s, reinterpret_cast<const bf16*>(x), feat, HW, C);
}

__global__ void fc_fwd_kernel(const float* __restrict__ feat, const float* __restrict__ W,
                              const float* __restrict__ b, float* __restrict__ logits, int D, int C)
{
    const int img = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = wave; k < C; k += 4) {
        float s = 0.f;
        for (int d = lane; d < D; d += 64) s += feat[(size_t)img * D + d] * W[(size_t)k * D + d];
        s = wave_sum(s);
        if (lane == 0) logits[(size_t)img * C + k] = s + b[k];
    }
}
void k_fc_fwd(const float* feat, const float* W, const float* b, float* logits, int imgs, int D, int C,
              hipStream_t s)
{
    hipLaunchKernelGGL(fc_fwd_kernel, dim3(imgs), dim3(256), 0, s, feat, W, b, logits, D, C);
}

// dW[k][d] = sum_img dz[img][k] * feat[img][d]: block = (class k, 64 feature columns), 4 image lanes folded in a
// fixed order (deterministic).  grid (C, ceil(D/64)) instead of one block per class: with 1024 images the old
// one-block-per-class form ran 1.2 ms on 5 of the 256 CUs.
__global__ void fc_bwd_w_kernel(const float* __restrict__ dz, const float* __restrict__ feat,
                                float* __restrict__ dW, float* __restrict__ db, int imgs, int D, int C)
{
    __shared__ float red[4][64];
    const int k = blockIdx.x;
    const int dl = threadIdx.x & 63, il = threadIdx.x >> 6;
    const int d = blockIdx.y * 64 + dl;
    float s = 0.f, sb = 0.f;
    if (d < D)
        for (int i = il; i < imgs; i += 4) s += dz[(size_t)i * C + k] * feat[(size_t)i * D + d];
    if (blockIdx.y == 0 && dl == 0)
        for (int i = il; i < imgs; i += 4) sb += dz[(size_t)i * C + k];
    red[il][dl] = s;
    __syncthreads();
    if (il == 0 && d < D) dW[(size_t)k * D + d] = ((red[0][dl] + red[1][dl]) + red[2][dl]) + red[3][dl];
    __syncthreads();
    if (blockIdx.y == 0) {
        if (dl == 0) red[il][0] = sb;
        __syncthreads();
        if (threadIdx.x == 0) db[k] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
    }
}
// dfeat (autograd path, fm_backward_grads): d loss / d feature, where the feature is the pooled tensor BEFORE the dropout
// multiplier (EfficientNet-B0's `feature`; ResNet-18 has no mask).  Null: the fused steps' arithmetic, unchanged.
template <typename T>
__global__ void fc_bwd_x_kernel(const float* __restrict__ dz, const float* __restrict__ W,
                                const float* __restrict__ mask, const float* __restrict__ dfeat, T* __restrict__ dout, int D,
                                int C, int HW)
{
    const int img = blockIdx.x;
    const float inv = 1.f / (float)HW;
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        float s = 0.f;
        for (int k = 0; k < C; ++k) s += dz[(size_t)img * C + k] * W[(size_t)k * D + d];
        if (dfeat) {                                       // d pooled = mask * (dz W) + dfeat, spread over HW
            if (mask) s *= mask[(size_t)img * D + d];
            s = (s + dfeat[(size_t)img * D + d]) * inv;
        } else {
            s *= inv;
            if (mask) s *= mask[(size_t)img * D + d];      // dropout multiplier on the pooled feature
        }
        for (int p = 0; p < HW; ++p) dout[((size_t)img * HW + p) * D + d] = (T)s;
    }
}
void k_fc_bwd(const float* dz, const float* feat, const float* W, const float* mask, float* dW, float* db,
              void* dout, int dt, int imgs, int D, int C, int HW, hipStream_t s, const float* dfeat)
{
    hipLaunchKernelGGL(fc_bwd_w_kernel, dim3(C, (D + 63) / 64), dim3(256), 0, s, dz, feat, dW, db, imgs, D, C);
    if (dt == DT_F32)
        hipLaunchKernelGGL(fc_bwd_x_kernel<float>, dim3(imgs), dim3(256), 0, s, dz, W, mask, dfeat, reinterpret_cast<float*>(dout), D,
                           C, HW);
    else
        hipLaunchKernelGGL(fc_bwd_x_kernel<bf16>, dim3(imgs), dim3(256), 0, s, dz, W, mask, dfeat, reinterpret_cast<bf16*>(dout), D,
                           C, HW);
}

// ------------------------------------------------------------ losses -----------
// BCEWithLogits with pos_weight: l = (1-y) z + lw * softplus(-z), lw = 1 + (pw-1) y
__device__ __forceinline__ float bce_logits(float z, float y, float pw, float* dz)
{
    const float lw = 1.f + (pw - 1.f) * y;
    const float sp = log1pf(expf(-fabsf(z))) + fmaxf(-z, 0.f);
    *dz = (1.f - y) - lw * (1.f - sigmoidf_(z));
    return (1.f - y) * z + lw * sp;
}
// F.binary_cross_entropy on p = sigmoid(z): value and d/dz through sigmoid
__device__ __forceinline__ float bce_prob(float z, float y, float* dz)
{
    const float p = sigmoidf_(z);
    const float lp = fmaxf(logf(p), -100.f), l1p = fmaxf(logf(1.f - p), -100.f);
    const float pq = p * (1.f - p);
    *dz = (p - y) / fmaxf(pq, 1e-12f) * pq;
    return -(y * lp + (1.f - y) * l1p);
}

__global__ void loss_bce_kernel(const float* __restrict__ z, const float* __restrict__ y, ClassVec pw, int B, int C,
                                float inv_norm, float* __restrict__ dz, float* __restrict__ loss)
{
    __shared__ float sh[4];
    float acc = 0.f;
    for (int i = threadIdx.x; i < B * C; i += 256) {
        float d;
        acc += bce_logits(z[i], y[i], pw.v[i % C], &d);
        dz[i] = d * inv_norm;
    }
    const float tot = block_sum(acc, sh);
    if (threadIdx.x == 0) *loss = tot * inv_norm;
}
void k_loss_bce(const float* z, const float* y, ClassVec pos_w, int B, int C, float inv_norm, float* dz,
                float* loss, hipStream_t s)
{
    hipLaunchKernelGGL(loss_bce_kernel, dim3(1), dim3(256), 0, s, z, y, pos_w, B, C, inv_norm, dz, loss);
}

// z,g: [2B,C] (view 1 rows then view 2 rows); y: [B,C]
__global__ void loss_stage1_kernel(const float* __restrict__ z, const float* __restrict__ g,
                                   const float* __restrict__ y, ClassVec active, int B, int C, float inv_sup,
                                   float inv_dis, float* __restrict__ dz, float* __restrict__ loss)
{
    __shared__ float sh[4];
    float sup = 0.f, dis = 0.f;
    for (int i = threadIdx.x; i < 2 * B * C; i += 256) {
        const int c = i % C, row = i / C;
        const int yr = row < B ? row : row - B;
        float d;
        if (active.v[c] != 0.f) {
            sup += 0.5f * bce_prob(z[i], y[yr * C + c], &d);
            dz[i] = 0.5f * d * inv_sup;
        } else {
            const float p = sigmoidf_(z[i]), q = sigmoidf_(g[i]);
            const float e = p - q;
            dis += 0.5f * e * e;
            dz[i] = e * p * (1.f - p) * inv_dis;
        }
    }
    const float s1 = block_sum(sup, sh);
    const float s2 = block_sum(dis, sh);
    if (threadIdx.x == 0) *loss = s1 * inv_sup + s2 * inv_dis;
}
void k_loss_stage1(const float* z, const float* g, const float* y, ClassVec active, int B, int C, float inv_sup,
                   float inv_dis, float* dz, float* loss, hipStream_t s)
{
    hipLaunchKernelGGL(loss_stage1_kernel, dim3(1), dim3(256), 0, s, z, g, y, active, B, C, inv_sup, inv_dis, dz,
                       loss);
}

__global__ void loss_stage2_kernel(const float* __restrict__ z, const float* __restrict__ y,
                                   const float* __restrict__ distill, int B, int C, float* __restrict__ dz,
                                   float* __restrict__ loss)
{
    __shared__ float sh[4];
    float cnt = 0.f;
    for (int i = threadIdx.x; i < B * C; i += 256) cnt += distill[i] != 0.f ? 0.f : 1.f;
    const float den = block_sum(cnt, sh);
    const float inv = 1.f / den;
    float acc = 0.f;
    for (int i = threadIdx.x; i < B * C; i += 256) {
        float d;
        const float l = bce_prob(z[i], y[i], &d);
        const float sup = distill[i] != 0.f ? 0.f : 1.f;
        acc += l * sup;
        dz[i] = d * sup * inv;
    }
    const float tot = block_sum(acc, sh);
    if (threadIdx.x == 0) *loss = tot / den;
}
void k_loss_stage2(const float* z, const float* y, const float* distill, int B, int C, float* dz, float* loss,
                   hipStream_t s)
{
    hipLaunchKernelGGL(loss_stage2_kernel, dim3(1), dim3(256), 0, s, z, y, distill, B, C, dz, loss);
}

// z: [2B,C] weak rows then strong rows
__global__ void loss_fixmatch_kernel(const float* __restrict__ z, const float* __restrict__ y, ClassVec pw,
                                     ClassVec pwu, ClassVec active, int B, int C, int n_neg, float inv_sup,
                                     int cls_minus_ann, float* __restrict__ dz, float* __restrict__ loss)
{
    __shared__ float sh[4];
    __shared__ unsigned char conf[2048];
    // confident rows: every missing-class prob > 0.8 or < 0.2
    float nconf = 0.f;
    for (int r = threadIdx.x; r < B; r += 256) {
        bool ok = true;
        for (int c = 0; c < C; ++c) {
            if (active.v[c] != 0.f) continue;
            const float p = sigmoidf_(z[r * C + c]);
            ok = ok && (p > 0.8f || p < 0.2f);
        }
        conf[r] = ok;
        nconf += ok ? 1.f : 0.f;
    }
    const float n_idx = block_sum(nconf, sh);      // also makes conf[] visible
    const bool use_unsup = n_idx > 0.f && n_neg > 0;
    const float inv_uns = use_unsup ? 1.f / (n_idx * (float)cls_minus_ann) : 0.f;
    float sup = 0.f, uns = 0.f;
    for (int i = threadIdx.x; i < B * C; i += 256) {
        const int c = i % C, r = i / C;
        float d, dzw = 0.f, dzs = 0.f;
        if (active.v[c] != 0.f) {
            sup += bce_logits(z[i], y[i], pw.v[c], &d);
            dzw = d * inv_sup;
        } else if (use_unsup && conf[r]) {
            const float hard = sigmoidf_(z[i]) > 0.5f ? 1.f : 0.f;
            uns += bce_logits(z[B * C + i], hard, pwu.v[c], &d);
            dzs = d * inv_uns;
        }
        dz[i] = dzw;
        dz[B * C + i] = dzs;
    }
    const float s1 = block_sum(sup, sh);
    const float s2 = block_sum(uns, sh);
    if (threadIdx.x == 0) *loss = s1 * inv_sup + s2 * inv_uns;
}
void k_loss_fixmatch(const float* z, const float* y, ClassVec pos_w, ClassVec pos_wu, ClassVec active, int B,
                     int C, int n_neg, float inv_sup, int n_cls_minus_ann, float* dz, float* loss, hipStream_t s)
{
    hipLaunchKernelGGL(loss_fixmatch_kernel, dim3(1), dim3(256), 0, s, z, y, pos_w, pos_wu, active, B, C, n_neg,
                       inv_sup, n_cls_minus_ann, dz, loss);
}

// ------------------------------------------------------------ FedLSR / FedIRM heads ---
// Two-view heads of train_FedLSR (utils/local_training.py:1294-1314) and train_FedIRM (:370-376, 421-452).  z [2B][C]: view 1
// rows, then view 2 rows (fm_forward_train's layout); every element of dz [2B][C] is written.  One block, no atomics.  The
// gradients are fp32 like every head's.  The loss VALUE is formed and summed in double (per thread, then a fixed tree) and
// rounded once: it costs a few microseconds of a step and makes the reported scalar the correctly rounded one.  The C x C
// relation sums are fp32, folded in LDS in a fixed order; the quotient and sigmoid on top of them (C x C values) are double.
__device__ __forceinline__ double sigmoid_d(double z) { return 1.0 / (1.0 + exp(-z)); }
// value of BCEWithLogits(pos_weight) in double (bce_logits' formula)
__device__ __forceinline__ double bce_logits_d(double z, float y, float pw)
{
    const double lw = 1.0 + ((double)pw - 1.0) * (double)y;
    return (1.0 - (double)y) * z + lw * (log1p(exp(-fabs(z))) + fmax(-z, 0.0));
}
__device__ __forceinline__ double block_sum_d(double v, double* sh /*[4]*/)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// FedLSR: mean BCEWithLogits(pos_weight)(pred_mix, y) + beta JS(q1, q2), both means over the B C elements.
//   p = mix1 s1 + mix2 s2, pred_mix = sigmoid(2 log(p / (1 - p))) = p^2 / (p^2 + (1 - p)^2), fed to the criterion as a LOGIT
//   (the reference does); d pred_mix / dp = 2 p (1 - p) / (p^2 + (1 - p)^2)^2.
//   q_v = clamp(sigmoid(3 z_v), 1e-6, 1), m = (q1 + q2) / 2, JS element = (q1 log(q1 / m) + q2 log(q2 / m)) / 2,
//   d / d q_v = log(q_v / m) / 2 (the m terms cancel); the clamp passes no gradient below 1e-6.
// The one deviation from torch's fp32 autograd: the rational form of pred_mix, with 1 - p formed as mix1 sigmoid(-z1) +
// mix2 sigmoid(-z2), stays finite where p rounds to 1 (torch forms 0 * inf in log(p / (1 - p)) and returns NaN); the derivative
// tends to 0 there.
__global__ void loss_fedlsr_kernel(const float* __restrict__ z, const float* __restrict__ y, ClassVec pw, int B, int C,
                                   float mix1, float mix2, float beta, float* __restrict__ dz, float* __restrict__ loss)
{
    __shared__ double shd[4];
    const int n = B * C;
    const float inv_n = 1.f / (float)n;
    double ce = 0.0, js = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float z1 = z[i], z2 = z[n + i];
        const float s1 = sigmoidf_(z1), s2 = sigmoidf_(z2), o1 = sigmoidf_(-z1), o2 = sigmoidf_(-z2);
        const float p = mix1 * s1 + mix2 * s2, q = mix1 * o1 + mix2 * o2;      // q = 1 - p without the cancellation
        const float den = p * p + q * q;                                       // >= 1/2 up to rounding: never 0
        const float pm = p * p / den;
        float g;
        bce_logits(pm, y[i], pw.v[i % C], &g);
        const float dp = g * (2.f * p * q / (den * den)) * inv_n;
        const float a1 = sigmoidf_(3.f * z1), a2 = sigmoidf_(3.f * z2);
        const float c1 = fmaxf(a1, 1e-6f), c2 = fmaxf(a2, 1e-6f);              // the upper clamp at 1 never binds
        const float m = 0.5f * (c1 + c2);
        const float l1 = logf(c1 / m), l2 = logf(c2 / m);
        {                                                                      // the value, in double
            const double S1 = sigmoid_d(z1), S2 = sigmoid_d(z2);
            const double P = (double)mix1 * S1 + (double)mix2 * S2, Q = (double)mix1 * (1.0 - S1) + (double)mix2 * (1.0 - S2);
            ce += bce_logits_d(P * P / (P * P + Q * Q), y[i], pw.v[i % C]);
            const double C1 = fmax(sigmoid_d(3.0 * z1), 1e-6), C2 = fmax(sigmoid_d(3.0 * z2), 1e-6), M = 0.5 * (C1 + C2);
            js += 0.5 * (C1 * log(C1 / M) + C2 * log(C2 / M));
        }
        const float k = 0.5f * beta * inv_n;
        const float d1 = a1 >= 1e-6f ? k * l1 * 3.f * a1 * sigmoidf_(-3.f * z1) : 0.f;
        const float d2 = a2 >= 1e-6f ? k * l2 * 3.f * a2 * sigmoidf_(-3.f * z2) : 0.f;
        dz[i] = dp * mix1 * s1 * o1 + d1;
        dz[n + i] = dp * mix2 * s2 * o2 + d2;
    }
    const double t1 = block_sum_d(ce, shd);
    const double t2 = block_sum_d(js, shd);
    if (threadIdx.x == 0) *loss = (float)((t1 + (double)beta * t2) / (double)n);
}
void k_loss_fedlsr(const float* z, const float* y, ClassVec pos_w, int B, int C, float mix1, float mix2, float beta, float* dz,
                   float* loss, hipStream_t s)
{
    hipLaunchKernelGGL(loss_fedlsr_kernel, dim3(1), dim3(256), 0, s, z, y, pos_w, B, C, mix1, mix2, beta, dz, loss);
}

// get_confuse_matrix (:73-81) for C classes (the reference hard-codes 8: identical at C = 8): row i, column j of the matrix is
// sigmoid((sum_b z1[b][j] lab[b][i]) / (sum_b lab[b][i] + 1e-8) / 2).  PSEUDO: lab[b][i] = sel[b] && sigmoid(z1[b][i]) > 0.5
// (the relation phase's pseudo-labels over the selected rows), else lab = y.  The 256 threads take min(C C, 256) pairs at a
// time; with fewer pairs than threads the rows b are dealt to 256 / pairs lanes and folded in lane order through LDS.
// emit(pair, sum, count) runs in one thread per pair.  Block-uniform control flow (barriers inside).
// one element of the relation matrix from its fp32 sums: the denominator is the fp32 sum + 1e-8 as the reference forms it
__device__ __forceinline__ float relation_prob(float S, float N) { return (float)sigmoid_d((double)S / (double)(N + 1e-8f) / 2.0); }

template <bool PSEUDO, typename Emit>
__device__ __forceinline__ void relation_sums(const float* __restrict__ z1, const float* __restrict__ y,
                                              const unsigned char* sel, int B, int C, float* red_s, float* red_n, Emit emit)
{
    const int P = C * C, Pc = P < 256 ? P : 256, L = 256 / Pc;
    const int pl = threadIdx.x % Pc, bl = threadIdx.x / Pc;
    for (int pair0 = 0; pair0 < P; pair0 += Pc) {
        const int pair = pair0 + pl;
        float s = 0.f, n = 0.f;
        if (bl < L && pair < P) {
            const int i = pair / C, j = pair % C;
            for (int b = bl; b < B; b += L) {
                float lab;
                if (PSEUDO) lab = (sel[b] && sigmoidf_(z1[b * C + i]) > 0.5f) ? 1.f : 0.f;
                else lab = y[b * C + i];
                s += z1[b * C + j] * lab;
                n += lab;
            }
        }
        red_s[threadIdx.x] = s;
        red_n[threadIdx.x] = n;
        __syncthreads();
        if (bl == 0 && pair < P) {
            float S = red_s[pl], N = red_n[pl];
            for (int l = 1; l < L; ++l) { S += red_s[l * Pc + pl]; N += red_n[l * Pc + pl]; }
            emit(pair, S, N);
        }
        __syncthreads();
    }
}

// FedIRM, supervised phase: sum over both views and the active classes of BCEWithLogits(pos_weight)(z_v, y) / sup_norm;
// rel_acc (may be null) += get_confuse_matrix(z_1, y), which carries no gradient
__global__ void loss_fedirm_sup_kernel(const float* __restrict__ z, const float* __restrict__ y, ClassVec pw, ClassVec active,
                                       int B, int C, float sup_norm, float* __restrict__ rel_acc, float* __restrict__ dz,
                                       float* __restrict__ loss)
{
    __shared__ double shd[4];
    __shared__ float red_s[256], red_n[256];
    const float inv_sup = 1.f / sup_norm;               // sup_norm = bs_norm annotation_num, an integer held exactly
    double sup = 0.0;
    for (int i = threadIdx.x; i < 2 * B * C; i += 256) {
        const int c = i % C, row = i / C;
        const int yr = row < B ? row : row - B;
        float d = 0.f;
        if (active.v[c] != 0.f) {
            bce_logits(z[i], y[yr * C + c], pw.v[c], &d);
            sup += bce_logits_d(z[i], y[yr * C + c], pw.v[c]);
            d *= inv_sup;
        }
        dz[i] = d;
    }
    if (rel_acc)
        relation_sums<false>(z, y, nullptr, B, C, red_s, red_n,
                             [&](int pair, float S, float N) { rel_acc[pair] += relation_prob(S, N); });
    const double tot = block_sum_d(sup, shd);
    if (threadIdx.x == 0) *loss = (float)(tot / (double)sup_norm);
}
void k_loss_fedirm_sup(const float* z, const float* y, ClassVec pos_w, ClassVec active, int B, int C, float sup_norm,
                       float* rel_acc, float* dz, float* loss, hipStream_t s)
{
    hipLaunchKernelGGL(loss_fedirm_sup_kernel, dim3(1), dim3(256), 0, s, z, y, pos_w, active, B, C, sup_norm, rel_acc, dz, loss);
}

// FedIRM, relation phase: the supervised term + cw sum (sigmoid z_1 - sigmoid z_t)^2 / bs_norm + cw kd(Q, T).
//   selected rows (:426-433): every probability of the row > 0.7 or < 0.3, and -sum_c (p log(p + 1e-6) + (1 - p) log(1 - p + 1e-6)) < 2;
//   Q = get_confuse_matrix(z_1[selected], sigmoid(z_1)[selected] > 0.5); no row selected: Q = 0.5 and no kd gradient
//   (decided here, on the device); kd (:109-113) = sum_ij (T - Q)(log T - log Q) / (2 C), both kl_div terms 'batchmean' over C rows;
//   d kd / d Q = (log(Q / T) + 1 - T / Q) / (2 C), d Q_ij / d z_1[b][j] = Q (1 - Q) / 2 lab[b][i] / (n_i + 1e-8).
// The selection and the pseudo-labels carry no gradient; zt [B][C] gets none.  rel_acc (may be null) += get_confuse_matrix(z_1, y).
__global__ void loss_fedirm_rel_kernel(const float* __restrict__ z, const float* __restrict__ zt, const float* __restrict__ y,
                                       ClassVec pw, ClassVec active, int B, int C, float sup_norm, float bs_norm, float cw,
                                       const float* __restrict__ target, float* __restrict__ rel_acc, float* __restrict__ dz,
                                       float* __restrict__ loss)
{
    __shared__ double shd[4];
    __shared__ float sh[4];
    __shared__ float red_s[256], red_n[256];
    __shared__ float G[FM_MAXC * FM_MAXC];      // d kd / d (the relation sum of pair (i, j))
    __shared__ unsigned char sel[2048];
    const float inv_sup = 1.f / sup_norm, inv_bs = 1.f / bs_norm;       // integers held exactly: the loss divides by them in double
    float nsel = 0.f;
    for (int r = threadIdx.x; r < B; r += 256) {
        bool ok = true;
        float unc = 0.f;
        for (int c = 0; c < C; ++c) {
            const float p = sigmoidf_(z[r * C + c]);
            ok = ok && (p > 0.7f || p < 0.3f);
            unc += p * logf(p + 1e-6f) + (1.f - p) * logf(1.f - p + 1e-6f);
        }
        ok = ok && (-unc < 2.0f);
        sel[r] = ok;
        nsel += ok ? 1.f : 0.f;
    }
    const bool any = block_sum(nsel, sh) > 0.f;             // also makes sel[] visible; block-uniform
    if (rel_acc)
        relation_sums<false>(z, y, nullptr, B, C, red_s, red_n,
                             [&](int pair, float S, float N) { rel_acc[pair] += relation_prob(S, N); });
    double kd = 0.0;
    const float inv_2c = 0.5f / (float)C;
    if (any) {
        relation_sums<true>(z, y, sel, B, C, red_s, red_n, [&](int pair, float S, float N) {
            const float den = N + 1e-8f;
            const double a = (double)S / (double)den / 2.0, Q = sigmoid_d(a), T = target[pair];
            kd += (Q - T) * log(Q / T);
            const float q = (float)Q, t = target[pair];
            G[pair] = (logf(q / t) + 1.f - t / q) * inv_2c * (q * (float)sigmoid_d(-a) * 0.5f) / den;
        });
    } else {
        for (int pair = threadIdx.x; pair < C * C; pair += 256) {
            const double T = target[pair];
            kd += (0.5 - T) * log(0.5 / T);
            G[pair] = 0.f;
        }
    }
    __syncthreads();
    double sup = 0.0, con = 0.0;
    for (int i = threadIdx.x; i < B * C; i += 256) {
        const int j = i % C, b = i / C;
        float d1 = 0.f, d2 = 0.f, d;
        if (active.v[j] != 0.f) {
            const float yy = y[i];
            bce_logits(z[i], yy, pw.v[j], &d);
            d1 = d * inv_sup;
            bce_logits(z[B * C + i], yy, pw.v[j], &d);
            d2 = d * inv_sup;
            sup += bce_logits_d(z[i], yy, pw.v[j]) + bce_logits_d(z[B * C + i], yy, pw.v[j]);
        }
        const float p = sigmoidf_(z[i]), e = p - sigmoidf_(zt[i]);
        {
            const double E = sigmoid_d(z[i]) - sigmoid_d(zt[i]);
            con += E * E;
        }
        d1 += cw * inv_bs * 2.f * e * p * sigmoidf_(-z[i]);
        if (any && sel[b]) {
            float g = 0.f;
            for (int k = 0; k < C; ++k)
                if (sigmoidf_(z[b * C + k]) > 0.5f) g += G[k * C + j];
            d1 += cw * g;
        }
        dz[i] = d1;
        dz[B * C + i] = d2;
    }
    const double t1 = block_sum_d(sup, shd);
    const double t2 = block_sum_d(con, shd);
    const double t3 = block_sum_d(kd, shd);
    if (threadIdx.x == 0)
        *loss = (float)(t1 / (double)sup_norm + (double)cw * (t2 / (double)bs_norm + t3 / (2.0 * (double)C)));
}
void k_loss_fedirm_rel(const float* z, const float* zt, const float* y, ClassVec pos_w, ClassVec active, int B, int C,
                       float sup_norm, float bs_norm, float cw, const float* target, float* rel_acc, float* dz, float* loss,
                       hipStream_t s)
{
    hipLaunchKernelGGL(loss_fedirm_rel_kernel, dim3(1), dim3(256), 0, s, z, zt, y, pos_w, active, B, C, sup_norm, bs_norm, cw,
                       target, rel_acc, dz, loss);
}

// ------------------------------------------------------------ RSCFed / FedNoRo / CBAFed heads ---
// Single-view heads of train_RSCFed (utils/local_training.py:719, 740-743), train_FedNoRo's warm-up (LA_KD.forward,
// utils/FedNoRo.py:35-38) and train_CBAFed (:247-269 warm-up, :303-333 stage 2).  z, dz [B][C]; every element of dz is written,
// exact zeros where an element is not in the loss.  One block, no atomics.  Value AND gradient are formed in double from the fp32
// logits and rounded once (B C elements: microseconds of a step); only CBAFed's threshold decisions are fp32 compares, as the
// trainer's torch code made them.
__device__ __forceinline__ int wave_sum_i(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
// BCEWithLogits(pos_weight) in double: the value, and d/dz = (1 - y) - lw sigmoid(-z)
__device__ __forceinline__ double bce_logits_dd(double z, float y, float pw, double* dz)
{
    const double lw = 1.0 + ((double)pw - 1.0) * (double)y;
    *dz = (1.0 - (double)y) - lw * sigmoid_d(-z);
    return (1.0 - (double)y) * z + lw * (log1p(exp(-fabs(z))) + fmax(-z, 0.0));
}

// RSCFed: sum_active BCEWithLogits(pos_weight)(z, y) / sup_norm + mean over the B n_miss missing elements of
// (sigmoid z - sigmoid zt)^2; zt gets no gradient
__global__ void loss_rscfed_kernel(const float* __restrict__ z, const float* __restrict__ zt, const float* __restrict__ y,
                                   ClassVec pw, ClassVec active, int B, int C, float sup_norm, int n_miss,
                                   float* __restrict__ dz, float* __restrict__ loss)
{
    __shared__ double shd[4];
    const double n_mse = (double)B * (double)n_miss;
    double sup = 0.0, con = 0.0;
    for (int i = threadIdx.x; i < B * C; i += 256) {
        const int c = i % C;
        double d;
        if (active.v[c] != 0.f) {
            sup += bce_logits_dd(z[i], y[i], pw.v[c], &d);
            d /= (double)sup_norm;
        } else {
            const double P = sigmoid_d(z[i]), E = P - sigmoid_d(zt[i]);
            con += E * E;
            d = 2.0 * E * (P * (1.0 - P)) / n_mse;
        }
        dz[i] = (float)d;
    }
    const double t1 = block_sum_d(sup, shd);
    const double t2 = block_sum_d(con, shd);
    if (threadIdx.x == 0) *loss = (float)(t1 / (double)sup_norm + t2 / n_mse);
}
void k_loss_rscfed(const float* z, const float* zt, const float* y, ClassVec pos_w, ClassVec active, int B, int C, float sup_norm,
                   int n_miss, float* dz, float* loss, hipStream_t s)
{
    hipLaunchKernelGGL(loss_rscfed_kernel, dim3(1), dim3(256), 0, s, z, zt, y, pos_w, active, B, C, sup_norm, n_miss, dz, loss);
}

// LA_KD: p = sigmoid(z), soft = sigmoid(zt / 0.8f);
//   (1 - w_kd) sum_active BCE(p, y) / (B n_act) + w_kd sum_missing (p - soft)^2 / (B n_miss), log clamped at -100.
// 1 - p is formed as torch forms it (1 - p, not sigmoid(-z)): where p rounds to 1 the log clamps at -100 and, like
// binary_cross_entropy's backward, the gradient (p - y) / max(p (1 - p), 1e-12) * p (1 - p) is 0.
__global__ void loss_lakd_kernel(const float* __restrict__ z, const float* __restrict__ zt, const float* __restrict__ y,
                                 ClassVec active, int B, int C, int n_act, float w_kd, float* __restrict__ dz,
                                 float* __restrict__ loss)
{
    __shared__ double shd[4];
    const double n_bce = (double)B * (double)n_act, n_kd = (double)B * (double)(C - n_act);
    const double wk = (double)w_kd, wb = 1.0 - (double)w_kd;
    double bce = 0.0, kd = 0.0;
    for (int i = threadIdx.x; i < B * C; i += 256) {
        const int c = i % C;
        const double P = sigmoid_d(z[i]), Q = 1.0 - P, PQ = P * Q;
        double d;
        if (active.v[c] != 0.f) {
            const double yy = y[i];
            bce -= yy * fmax(log(P), -100.0) + (1.0 - yy) * fmax(log(Q), -100.0);
            d = wb * ((P - yy) / fmax(PQ, 1e-12) * PQ) / n_bce;
        } else {
            const double E = P - sigmoid_d((double)(zt[i] / 0.8f));
            kd += E * E;
            d = wk * 2.0 * E * PQ / n_kd;
        }
        dz[i] = (float)d;
    }
    const double t1 = block_sum_d(bce, shd);
    const double t2 = block_sum_d(kd, shd);
    if (threadIdx.x == 0) *loss = (float)(wk * (t2 / n_kd) + wb * (t1 / n_bce));
}
void k_loss_lakd(const float* z, const float* zt, const float* y, ClassVec active, int B, int C, int n_act, float w_kd, float* dz,
                 float* loss, hipStream_t s)
{
    hipLaunchKernelGGL(loss_lakd_kernel, dim3(1), dim3(256), 0, s, z, zt, y, active, B, C, n_act, w_kd, dz, loss);
}

// CBAFed.  Warm-up (STAGE2 false): the active-class BCEWithLogits(pos_weight) / sup_norm; pos_weight [C] is only read, counts
// is not touched.  Stage 2: pass 1 counts, per missing class i, hi = sigmoid(z) > tao[i], lo = sigmoid(z) < 1.f - tao[i] and their
// union over the B rows (integers: wave w takes classes w, w + 4, ..., its lanes the rows); one thread per class then writes
// pos_weight[i] = noise == 0 ? 1 : (float)((double)(noise + clean) / noise) and adds to counts [C + 1] (int64): n_i per missing
// class, B per active class, and their total (sum n_i + B annotation_num) in counts[C].  Pass 2 forms the loss with the NEW
// weights: the active term, plus per missing class with n_i > 0 the sum over its hi / lo rows of l / n_i, the label 1 where hi
// (in registers: y is not written).  The decisions of pass 2 re-evaluate pass 1's fp32 expressions, so they agree.
template <bool STAGE2>
__global__ void loss_cbafed_kernel(const float* __restrict__ z, const float* __restrict__ y, ClassVec active, ClassVec tao,
                                   int B, int C, float sup_norm, int annotation_num, float* __restrict__ pos_weight,
                                   long long* __restrict__ counts, float* __restrict__ dz, float* __restrict__ loss)
{
    __shared__ double shd[4];
    __shared__ int n_hi[FM_MAXC], n_lo[FM_MAXC], n_un[FM_MAXC];
    __shared__ float pw[FM_MAXC];
    if (STAGE2) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        for (int c = wave; c < C; c += 4) {
            int h = 0, l = 0, u = 0;
            if (active.v[c] == 0.f) {
                const float t = tao.v[c], t1 = 1.f - t;
                for (int r = lane; r < B; r += 64) {
                    const float p = sigmoidf_(z[r * C + c]);
                    const bool hi = p > t, lo = p < t1;
                    h += hi; l += lo; u += (hi || lo);
                }
            }
            h = wave_sum_i(h); l = wave_sum_i(l); u = wave_sum_i(u);
            if (lane == 0) { n_hi[c] = h; n_lo[c] = l; n_un[c] = u; }
        }
        __syncthreads();
    }
    if (threadIdx.x < C) {
        const int c = threadIdx.x;
        float w = pos_weight[c];
        if (STAGE2) {
            if (active.v[c] == 0.f) {
                w = n_hi[c] == 0 ? 1.f : (float)((double)(n_hi[c] + n_lo[c]) / (double)n_hi[c]);
                pos_weight[c] = w;
                counts[c] += n_un[c];
            } else counts[c] += B;
        }
        pw[c] = w;
    }
    __syncthreads();
    if (STAGE2 && threadIdx.x == 0) {
        long long tot = (long long)B * annotation_num;
        for (int c = 0; c < C; ++c)
            if (active.v[c] == 0.f) tot += n_un[c];
        counts[C] += tot;
    }
    double acc = 0.0;
    for (int i = threadIdx.x; i < B * C; i += 256) {
        const int c = i % C;
        double d = 0.0;
        if (active.v[c] != 0.f) {
            acc += bce_logits_dd(z[i], y[i], pw[c], &d) / (double)sup_norm;
            d /= (double)sup_norm;
        } else if (STAGE2) {
            const float p = sigmoidf_(z[i]);
            const bool hi = p > tao.v[c], lo = p < 1.f - tao.v[c];
            if (hi || lo) {
                const double n = (double)n_un[c];
                acc += bce_logits_dd(z[i], hi ? 1.f : y[i], pw[c], &d) / n;
                d /= n;
            }
        }
        dz[i] = (float)d;
    }
    const double tot = block_sum_d(acc, shd);
    if (threadIdx.x == 0) *loss = (float)tot;
}
void k_loss_cbafed(const float* z, const float* y, ClassVec active, const ClassVec* tao, int B, int C, float sup_norm,
                   int annotation_num, float* pos_weight, int64_t* counts, float* dz, float* loss, hipStream_t s)
{
    if (tao)
        hipLaunchKernelGGL(loss_cbafed_kernel<true>, dim3(1), dim3(256), 0, s, z, y, active, *tao, B, C, sup_norm, annotation_num,
                           pos_weight, reinterpret_cast<long long*>(counts), dz, loss);
    else
        hipLaunchKernelGGL(loss_cbafed_kernel<false>, dim3(1), dim3(256), 0, s, z, y, active, ClassVec{}, B, C, sup_norm,
                           annotation_num, pos_weight, reinterpret_cast<long long*>(counts), dz, loss);
}

// ------------------------------------------------------------ RoFL head ---------
// train_RoFL's batch (utils/local_training.py:524-572, 582-626) in three launches on one stream: no host read, no atomics, the
// same bits from run to run.  z, y [B][C], feat [B][D] (the train forward's pooled feature, a constant of the loss),
// fk [2C][D] the client's centroids (row 2c + t: class c, label value t), D a multiple of 4.
//   rofl_rows_kernel      one wave per row: the row's small-loss key sum_c BCEWithLogits(pos_weight)(z, y) in double, the
//                         cosines of the row's feature with every centroid (fp32, lane-strided then a fixed butterfly: they
//                         only decide the vote), and per class the squared distance to the centroid of the row's own label
//                         (double: it is part of the loss value)
//   rofl_select_kernel    one block: rank by counting (ties to the lower row, NaN keys last), keep the n_keep smallest; the
//                         vote, the mask, the label table, the loss and dz (double, rounded once; exact 0 off the kept rows)
//   rofl_centroid_kernel  one block per centroid row: the kept rows' feature mean in row order, s = cos(fk, mean) and the blend
//                         fk <- (1 - s^2) fk + s^2 mean, in double, rounded once -- launched last: the loss reads the old fk.
// Cosine is a.b / (|a| |b|), and exactly 0 when a norm is 0.
__global__ void rofl_rows_kernel(const float* __restrict__ z, const float* __restrict__ y, const float* __restrict__ feat,
                                 const float* __restrict__ fk, ClassVec pw, int B, int C, int D, double* __restrict__ rowloss,
                                 float* __restrict__ cosv, double* __restrict__ dist)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= B) return;                                     // wave-uniform
    double l = 0.0;
    if (lane < C) {
        l = bce_logits_d(z[(size_t)i * C + lane], y[(size_t)i * C + lane], pw.v[lane]);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) l += __shfl_xor(l, d);
    if (lane == 0) rowloss[i] = l;
    const float4* f = reinterpret_cast<const float4*>(feat + (size_t)i * D);
    const int D4 = D >> 2;
    float ff = 0.f;
    for (int d = lane; d < D4; d += 64) {
        const float4 x = f[d];
        ff += (x.x * x.x + x.y * x.y) + (x.z * x.z + x.w * x.w);
    }
    const float fn = sqrtf(wave_sum(ff));
    for (int c = 0; c < C; ++c) {
        const float4* p0 = reinterpret_cast<const float4*>(fk + (size_t)(2 * c) * D);
        const float4* p1 = p0 + D4;
        const bool one = y[(size_t)i * C + c] != 0.f;
        float d0 = 0.f, d1 = 0.f, n0 = 0.f, n1 = 0.f;
        double dd = 0.0;
        for (int d = lane; d < D4; d += 64) {
            const float4 x = f[d], a = p0[d], b = p1[d];
            d0 += (x.x * a.x + x.y * a.y) + (x.z * a.z + x.w * a.w);
            d1 += (x.x * b.x + x.y * b.y) + (x.z * b.z + x.w * b.w);
            n0 += (a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w);
            n1 += (b.x * b.x + b.y * b.y) + (b.z * b.z + b.w * b.w);
            const float4 t = one ? b : a;
            const double e0 = (double)x.x - (double)t.x, e1 = (double)x.y - (double)t.y, e2 = (double)x.z - (double)t.z,
                         e3 = (double)x.w - (double)t.w;
            dd += (e0 * e0 + e1 * e1) + (e2 * e2 + e3 * e3);
        }
        d0 = wave_sum(d0); d1 = wave_sum(d1);
        n0 = sqrtf(wave_sum(n0)); n1 = sqrtf(wave_sum(n1));
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) dd += __shfl_xor(dd, d);
        if (lane == 0) {
            cosv[(size_t)i * 2 * C + 2 * c] = (fn == 0.f || n0 == 0.f) ? 0.f : d0 / (fn * n0);
            cosv[(size_t)i * 2 * C + 2 * c + 1] = (fn == 0.f || n1 == 0.f) ? 0.f : d1 / (fn * n1);
            dist[(size_t)i * C + c] = dd;
        }
    }
}

// key order of the small-loss selection: ascending, NaN last, ties to the lower row
__device__ __forceinline__ bool rofl_before(double a, int ia, double b, int ib)
{
    const bool an = a != a, bn = b != b;
    if (an || bn) return an == bn ? ia < ib : bn;
    return a < b || (a == b && ia < ib);
}

// keepw [B]: bit 0 kept, bit 1 mask (the workspace rofl_centroid_kernel reads; keep_out, may be null, gets a copy).
// pseudo uint8 [N][C]: rows item[i] of the kept rows are read and, with write_labels, written.  The items of one batch are
// distinct (a loader without replacement), so each thread owns its rows' table entries; an item outside [0, N) is never
// dereferenced (the row then stands on its own label).
__global__ void rofl_select_kernel(const float* __restrict__ z, const float* __restrict__ y, const int* __restrict__ item,
                                   const double* __restrict__ rowloss, const float* __restrict__ cosv,
                                   const double* __restrict__ dist, ClassVec pw, int B, int C, int D, int n_keep, int N,
                                   double lam_cen, double lam_e, int write_labels, unsigned char* __restrict__ pseudo,
                                   int* __restrict__ keepw, int* __restrict__ keep_out, float* __restrict__ dz,
                                   float* __restrict__ loss)
{
    __shared__ double shd[4];
    for (int i = threadIdx.x; i < B; i += 256) {
        const double li = rowloss[i];
        int rank = 0;
        for (int j = 0; j < B; ++j) rank += rofl_before(rowloss[j], j, li, i);
        int flags = 0;
        if (rank < n_keep) {
            bool agree = true;
            for (int c = 0; c < C; ++c) {
                const float vote = cosv[(size_t)i * 2 * C + 2 * c + 1] > cosv[(size_t)i * 2 * C + 2 * c] ? 1.f : 0.f;
                agree = agree && vote == y[(size_t)i * C + c];
            }
            flags = 1 | (agree ? 2 : 0);
            const int it = item[i];
            if (write_labels && it >= 0 && it < N)
                for (int c = 0; c < C; ++c) pseudo[(size_t)it * C + c] = y[(size_t)i * C + c] != 0.f ? 1 : 0;
        }
        keepw[i] = flags;
        if (keep_out) keep_out[i] = flags;
    }
    __syncthreads();                                        // keepw and the table rows written above are visible to the block
    const double nk = (double)n_keep, inv = 1.0 / (nk * (double)C);
    double lc = 0.0, le = 0.0, cen = 0.0;
    for (int e = threadIdx.x; e < B * C; e += 256) {
        const int i = e / C, c = e % C;
        const int flags = keepw[i];
        double g = 0.0;
        if (flags & 1) {
            const int it = item[i];
            float lab = y[e];
            if (!(flags & 2) && it >= 0 && it < N) lab = (float)pseudo[(size_t)it * C + c];
            const double zz = z[e], p = sigmoid_d(zz), q = sigmoid_d(-zz);
            lc += bce_logits_dd(zz, lab, pw.v[c], &g);
            le += (log1p(exp(-fabs(zz))) + fmax(zz, 0.0)) - zz * p;          // H = softplus(z) - z p, finite everywhere
            g = (g - lam_e * zz * p * q) * inv;
            if (flags & 2) cen += dist[e];
        }
        dz[e] = (float)g;
    }
    const double t1 = block_sum_d(lc, shd);
    const double t2 = block_sum_d(le, shd);
    const double t3 = block_sum_d(cen, shd);
    if (threadIdx.x == 0) *loss = (float)(t1 * inv + lam_cen * (t3 / (nk * (double)D) / (double)C) + lam_e * (t2 * inv));
}

__global__ void rofl_centroid_kernel(const float* __restrict__ y, const float* __restrict__ feat, const int* __restrict__ keepw,
                                     int B, int C, int D, float* __restrict__ fk)
{
    extern __shared__ double rofl_mean[];                   // [D]
    __shared__ double shd[4];
    const int r = blockIdx.x, c = r >> 1;
    const float want = (float)(r & 1);
    int n = 0;
    for (int i = 0; i < B; ++i) n += (keepw[i] & 1) && y[(size_t)i * C + c] == want;        // block-uniform
    const double den = n ? (double)n : 1.0;
    float* row = fk + (size_t)r * D;
    double ab = 0.0, aa = 0.0, bb = 0.0;
    for (int d = threadIdx.x; d < D; d += 256) {
        double s = 0.0;
        for (int i = 0; i < B; ++i)
            if ((keepw[i] & 1) && y[(size_t)i * C + c] == want) s += (double)feat[(size_t)i * D + d];
        const double m = s / den, a = row[d];
        rofl_mean[d] = m;
        ab += a * m; aa += a * a; bb += m * m;
    }
    ab = block_sum_d(ab, shd);
    aa = block_sum_d(aa, shd);
    bb = block_sum_d(bb, shd);
    const double s = (aa == 0.0 || bb == 0.0) ? 0.0 : ab / (sqrt(aa) * sqrt(bb)), s2 = s * s;
    for (int d = threadIdx.x; d < D; d += 256) row[d] = (float)((1.0 - s2) * (double)row[d] + s2 * rofl_mean[d]);
}

void k_loss_rofl(const float* z, const float* feat, const float* y, const int* item, int B, int C, int D, int n_keep,
                 ClassVec pos_w, float lambda_cen, float lambda_e, int write_labels, float* centroids, unsigned char* pseudo,
                 int N, double* ws_rowloss, float* ws_cos, double* ws_dist, int* ws_keep, int* keep_out, float* dz, float* loss,
                 hipStream_t s)
{
    hipLaunchKernelGGL(rofl_rows_kernel, dim3(cdiv(B, 4)), dim3(256), 0, s, z, y, feat, centroids, pos_w, B, C, D, ws_rowloss,
                       ws_cos, ws_dist);
    hipLaunchKernelGGL(rofl_select_kernel, dim3(1), dim3(256), 0, s, z, y, item, ws_rowloss, ws_cos, ws_dist, pos_w, B, C, D,
                       n_keep, N, (double)lambda_cen, (double)lambda_e, write_labels, pseudo, ws_keep, keep_out, dz, loss);
    hipLaunchKernelGGL(rofl_centroid_kernel, dim3(2 * C), dim3(256), (size_t)D * sizeof(double), s, y, feat, ws_keep, B, C, D,
                       centroids);
}

// ------------------------------------------------------------ prototypes -------
// grid = 2C blocks: block r = 2c+v sums feature rows whose label[c] == v (active c),
// and (v == 0, negative c) counts confident probabilities.  One block per output
// row -> no atomics, fixed order.
__global__ void proto_accumulate_kernel(const float* __restrict__ feat, const float* __restrict__ logits,
                                        const float* __restrict__ labels, int B, int D, int C, ClassVec active,
                                        ClassVec negative, float L, float U, float* __restrict__ psum,
                                        int64_t* __restrict__ pcnt, int64_t* __restrict__ tcnt)
{
    __shared__ float sh[4];
    const int r = blockIdx.x, c = r >> 1, v = r & 1;
    if (active.v[c] != 0.f) {
        const float want = (float)v;
        for (int d = threadIdx.x; d < D; d += 256) {
            float s = 0.f;
            for (int b = 0; b < B; ++b)
                if (labels[(size_t)b * C + c] == want) s += feat[(size_t)b * D + d];
            psum[(size_t)r * D + d] += s;
        }
        float n = 0.f;
        for (int b = threadIdx.x; b < B; b += 256) n += labels[(size_t)b * C + c] == want ? 1.f : 0.f;
        n = block_sum(n, sh);
        if (threadIdx.x == 0) pcnt[r] += (int64_t)n;
    }
    if (v == 0 && negative.v[c] != 0.f) {
        float n = 0.f;
        for (int b = threadIdx.x; b < B; b += 256) {
            const float p = sigmoidf_(logits[(size_t)b * C + c]);
            n += (p < L || p > U) ? 1.f : 0.f;
        }
        n = block_sum(n, sh);
        if (threadIdx.x == 0) tcnt[c] += (int64_t)n;
    }
}
void k_proto_accumulate(const float* feat, const float* logits, const float* labels, int B, int D, int C,
                        ClassVec active, ClassVec negative, float L, float U, float* psum, int64_t* pcnt,
                        int64_t* tcnt, hipStream_t s)
{
    hipLaunchKernelGGL(proto_accumulate_kernel, dim3(2 * C), dim3(256), 0, s, feat, logits, labels, B, D, C, active,
                       negative, L, U, psum, pcnt, tcnt);
}

// ------------------------------------------------------------ cosine tagging ---
// one wave per sample; prototypes' norms recomputed per wave (2*ncls rows of D, L2-resident)
__global__ void cos_tag_kernel(const float* __restrict__ feat, int64_t N, int D, const float* __restrict__ proto,
                               const int* __restrict__ classes, int ncls, float* __restrict__ sim)
{
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const float* f = feat + n * D;
    float ff = 0.f;
#pragma unroll 8
    for (int d = lane; d < D; d += 64) ff += f[d] * f[d];
    const float fn = sqrtf(wave_sum(ff));
    for (int k = 0; k < ncls; ++k) {
        const float* p0 = proto + (size_t)(2 * classes[k]) * D;
        const float* p1 = p0 + D;
        float d0 = 0.f, d1 = 0.f, n0 = 0.f, n1 = 0.f;
#pragma unroll 4
        for (int d = lane; d < D; d += 64) {
            const float x = f[d], a = p0[d], b = p1[d];
            d0 += x * a; d1 += x * b; n0 += a * a; n1 += b * b;
        }
        d0 = wave_sum(d0); d1 = wave_sum(d1);
        n0 = sqrtf(wave_sum(n0)); n1 = sqrtf(wave_sum(n1));
        if (lane == 0) sim[(size_t)k * N + n] = d0 * (1.f / (fn * n0)) - d1 * (1.f / (fn * n1));
    }
}
void k_cos_tag(const float* feat, int64_t N, int D, const float* proto, const int* classes, int ncls, float* sim,
               hipStream_t s)
{
    hipLaunchKernelGGL(cos_tag_kernel, dim3(cdiv(N, 4)), dim3(256), 0, s, feat, N, D, proto, classes, ncls, sim);
}

__global__ void count_sign_kernel(const float* __restrict__ sim, int64_t N, int* __restrict__ counts)
{
    __shared__ float sh[4];
    float a = 0.f, b = 0.f;
    for (int64_t i = threadIdx.x; i < N; i += 256) {
        const float v = sim[i];
        a += v >= 0.f ? 1.f : 0.f;
        b += v < 0.f ? 1.f : 0.f;
    }
    a = block_sum(a, sh);
    b = block_sum(b, sh);
    if (threadIdx.x == 0) { counts[0] = (int)a; counts[1] = (int)b; }
}
void k_count_sign(const float* sim, int64_t N, int* counts, hipStream_t s)
{
    hipLaunchKernelGGL(count_sign_kernel, dim3(1), dim3(256), 0, s, sim, N, counts);
}

// rank of element i in a stable descending / ascending sort (first position wins ties).  A NaN element is left out: it is
// ranked nowhere and selects nothing (every comparison with it is false, so the others' ranks are those of the row without it;
// its own rank would come out 0 and race with the true largest / smallest for slot 0)
__global__ void rank_select_kernel(const float* __restrict__ sim, int64_t N, int ktop, int kbot,
                                   int* __restrict__ top, int* __restrict__ bot)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float v = sim[i];
    if (v != v) return;
    int rd = 0, ra = 0;
    for (int64_t j = 0; j < N; ++j) {
        const float u = sim[j];
        rd += (u > v) || (u == v && j < i);
        ra += (u < v) || (u == v && j < i);
    }
    if (rd < ktop) top[rd] = (int)i;
    if (ra < kbot) bot[ra] = (int)i;
}
// ---- every missing class of a round in one launch pair (fm_select_topk_rows) ----------------------------------------------
// sim [ncls][N]; class k's pool = rows[k*stride .. + pn[k]) (positions into its sim row, pool order), or all N rows when rows
// is null.  counts[k] = (#(sim >= 0), #(sim < 0)) over the pool (NaN in neither, like utils/local_training.py:1061-1066)
__global__ void count_sign_rows_kernel(const float* __restrict__ sim, int64_t N, const int* __restrict__ rows,
                                       const int* __restrict__ pn, int stride, int* __restrict__ counts)
{
    __shared__ float sh[4];
    const int k = blockIdx.x;
    const int n = pn[k];
    const float* sr = sim + (size_t)k * N;
    float a = 0.f, b = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float v = sr[rows ? rows[(size_t)k * stride + i] : i];
        a += v >= 0.f ? 1.f : 0.f;
        b += v < 0.f ? 1.f : 0.f;
    }
    a = block_sum(a, sh);
    b = block_sum(b, sh);
    if (threadIdx.x == 0) { counts[2 * k] = (int)a; counts[2 * k + 1] = (int)b; }
}
// stable ranks inside each pool; ktop / kbot = int(thr * count) with the reference's double arithmetic and truncation (:1069-1070)
__global__ void rank_select_rows_kernel(const float* __restrict__ sim, int64_t N, const int* __restrict__ rows,
                                        const int* __restrict__ pn, int stride, const int* __restrict__ counts, double clean_thr,
                                        double noise_thr, int cap, int* __restrict__ top, int* __restrict__ bot)
{
    const int k = blockIdx.y;
    const int n = pn[k];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int ktop = (int)(1 * clean_thr * counts[2 * k]), kbot = (int)(1 * noise_thr * counts[2 * k + 1]);
    if (ktop == 0 && kbot == 0) return;
    const float* sr = sim + (size_t)k * N;
    const int* rk = rows ? rows + (size_t)k * stride : nullptr;
    const float v = sr[rk ? rk[i] : i];
    if (v != v) return;                                   // NaN: left out, as in rank_select_kernel
    int rd = 0, ra = 0;
    for (int j = 0; j < n; ++j) {
        const float u = sr[rk ? rk[j] : j];
        rd += (u > v) || (u == v && j < i);
        ra += (u < v) || (u == v && j < i);
    }
    if (rd < ktop && rd < cap) top[(size_t)k * cap + rd] = i;
    if (ra < kbot && ra < cap) bot[(size_t)k * cap + ra] = i;
}
void k_select_rows(const float* sim, int64_t N, int ncls, const int* rows, const int* pn, int stride, int maxn, double clean_thr,
                   double noise_thr, int cap, int* counts, int* top, int* bot, hipStream_t s)
{
    hipLaunchKernelGGL(count_sign_rows_kernel, dim3(ncls), dim3(256), 0, s, sim, N, rows, pn, stride, counts);
    if (maxn > 0)
        hipLaunchKernelGGL(rank_select_rows_kernel, dim3(cdiv(maxn, 256), ncls), dim3(256), 0, s, sim, N, rows, pn, stride, counts,
                           clean_thr, noise_thr, cap, top, bot);
}

void k_rank_select(const float* sim, int64_t N, int ktop, int kbot, int* top, int* bot, hipStream_t s)
{
    hipLaunchKernelGGL(rank_select_kernel, dim3(cdiv(N, 256)), dim3(256), 0, s, sim, N, ktop, kbot, top, bot);
}

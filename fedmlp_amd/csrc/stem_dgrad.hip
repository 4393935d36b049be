// Data gradients of the two stems: d loss / d image for the autograd path (fm_backward_grads_x).  The fused steps never
// differentiate with respect to images and launch nothing from this file.
//
// ResNet-18, 7x7 / stride 2 / pad 3, 64 -> 3 (stem_dgrad_kernel)
//   Site (i, j) of the half-resolution grid owns the four input pixels (2i + ph, 2j + pw).  Their 12 values (parity class x
//   channel) all read the same 4 x 4 window of dy, rows i - 1 .. i + 2 and columns j - 1 .. j + 2:
//       dx[2i + ph][2j + pw][ci] = sum_{dh, dw, co} dy[i + dh - 1][j + dw - 1][co] * w[co][5 - 2 dh + ph][5 - 2 dw + pw][ci]
//   (a tap index of -1 does not exist: the even classes have three taps per axis, the odd ones four).  So the whole gradient is
//   ONE GEMM, M = sites, N = 16 (12 used), K = 16 window taps x 64 channels = 1024, against a constant 1024 x 16 matrix:
//   the 7x7 taps scattered by parity class, zero elsewhere (49 of 64 taps x 12 of 16 columns: 57 % useful MACs).  dy is read once,
//   nothing is atomic, every dx element is written exactly once.
//   Arithmetic: v_mfma_f32_16x16x4_f32, i.e. exact fp32 products and fp32 accumulation, for every handle whatever
//   fm_config.reserved[2] says (the bf16 partial products of split3.h would need planes of dy nobody else reads).
//   A block is persistent: it keeps the whole B matrix in LDS (64 KB, in the order the lanes read it: one ds_read_b128 feeds
//   four MFMAs) and walks tiles of 8 x 16 sites.  A tile's 11 x 19 window pixels are fetched into registers while the previous
//   tile is multiplied, then staged in LDS (rows of 68 floats: the 16 pixel lanes of a fragment read fall on different banks).
//   Wave w owns site rows 2w, 2w + 1 of the tile: two independent accumulators share each B fragment.  Inside a window tap the
//   K order is permuted so that a lane's four k-slices are 16 CONSECUTIVE channels: MFMA (m4, c) takes channel 16 q + 4 m4 + c
//   from k-lane q.  The result goes through a wave-private LDS tile so that every store is a 128-byte run of one image row.
//   Roofline at bs 128 x 224^2: 52.6 GFLOP issued on the fp32 matrix pipe (155 TF) = 0.34 ms; HBM (411 MB in, 77 MB out) would
//   be 0.1 ms -- the kernel is bound by the fp32 matrix pipe, not by memory.
//
// EfficientNet-B0, 3x3 / stride 2 / TF-"same", 32 -> 3 (eff_stem_dgrad_kernel): 65 MFLOP per image against 1.6 MB of dy, plain
//   vector FMAs, one thread per input pixel, dy in the engine's storage type, dx fp32.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int SD_TI = 8, SD_TJ = 16;                  // sites per tile
constexpr int SD_R = SD_TI + 3, SD_C = SD_TJ + 3;     // window pixels per tile
constexpr int SD_PS = 68;                             // floats per staged pixel (64 + 4: bank spread)
constexpr int SD_B = 16 * 4 * 64 * 4;                 // B matrix floats: [tap][m4][lane][c]
constexpr int SD_A = SD_R * SD_C * SD_PS;
constexpr int SD_O = 4 * 12 * 32;                     // per wave: [site row 2][ph 2][ci 3][32 columns]
constexpr int SD_LDS = (SD_B + SD_A + SD_O) * 4;
constexpr int SD_NF4 = SD_R * SD_C * 16;              // 16-byte pieces of a tile's window
constexpr int SD_PRE = (SD_NF4 + 255) / 256;

// B in the order the lanes read it: element ((tap * 4 + m4) * 64 + lane) * 4 + c  =  Bmat[k = (tap, co)][n], lane = 16 q + n,
// co = 16 q + 4 m4 + c, n = (2 ph + pw) * 3 + ci, tap = 4 dh + dw.  w is the engine's stem weight [64][Kw], k = (kh * kw_p + kw) * cin_p + ci.
__global__ void stem_dgrad_pack_kernel(const float* __restrict__ w, float* __restrict__ out, int Kw, int kw_p, int cin_p)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= SD_B) return;
    const int c = idx & 3, lane = (idx >> 2) & 63, m4 = (idx >> 8) & 3, tap = idx >> 10;
    const int dh = tap >> 2, dw = tap & 3, q = lane >> 4, n = lane & 15;
    const int co = 16 * q + 4 * m4 + c;
    float v = 0.f;
    if (n < 12) {
        const int cls = n / 3, ci = n % 3, ph = cls >> 1, pw = cls & 1;
        const int kh = 5 - 2 * dh + ph, kw = 5 - 2 * dw + pw;
        if (kh >= 0 && kh < 7 && kw >= 0 && kw < 7) v = w[(size_t)co * Kw + (kh * kw_p + kw) * cin_p + ci];
    }
    out[idx] = v;
}

// NHWC_OUT: dx [imgs][H][W][3] (the fm_debug_conv convention) instead of [imgs][3][H][W]
template <bool NHWC_OUT>
__global__ __launch_bounds__(256) void stem_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ Bp,
                                                         float* __restrict__ dx, int imgs, int Ho, int Wo, int H, int W)
{
    extern __shared__ __attribute__((aligned(16))) float sd_lds[];
    float* Bs = sd_lds;
    float* As = sd_lds + SD_B;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* Os = sd_lds + SD_B + SD_A + wave * (12 * 32);

    for (int e = tid; e < SD_B / 4; e += 256) reinterpret_cast<f32x4*>(Bs)[e] = reinterpret_cast<const f32x4*>(Bp)[e];

    const int nTi = (Ho + SD_TI - 1) / SD_TI, nTj = (Wo + SD_TJ - 1) / SD_TJ;
    const long long ntiles = (long long)imgs * nTi * nTj;
    f32x4 pre[SD_PRE];
    auto fetch = [&](long long t) {
        const int tj = (int)(t % nTj), ti = (int)((t / nTj) % nTi), img = (int)(t / ((long long)nTj * nTi));
        const int oh0 = ti * SD_TI - 1, ow0 = tj * SD_TJ - 1;
#pragma unroll
        for (int it = 0; it < SD_PRE; ++it) {
            const int e = it * 256 + tid;
            const int pix = e >> 4, c4 = e & 15;
            const int r = pix / SD_C, c = pix - r * SD_C;
            const int oh = oh0 + r, ow = ow0 + c;
            const bool ok = e < SD_NF4 && oh >= 0 && oh < Ho && ow >= 0 && ow < Wo;
            const size_t off = ok ? (((size_t)img * Ho + oh) * Wo + ow) * 64 + 4 * c4 : 0;
            pre[it] = ld4z(dy + off, ok);
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int it = 0; it < SD_PRE; ++it) {
            const int e = it * 256 + tid;
            if (e < SD_NF4) st4(As + (e >> 4) * SD_PS + 4 * (e & 15), pre[it]);
        }
    };

    long long t = blockIdx.x;
    if (t < ntiles) fetch(t);
    const int p = lane & 15, q = lane >> 4;
    for (; t < ntiles; t += gridDim.x) {
        __syncthreads();                 // the previous tile's reads of As are done (first pass: Bs is written)
        stage();
        __syncthreads();
        const long long tn = t + gridDim.x;
        if (tn < ntiles) fetch(tn);      // in flight under the MFMAs below

        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        const float* a_base = As + ((2 * wave) * SD_C + p) * SD_PS + 16 * q;
        const f32x4* b_base = reinterpret_cast<const f32x4*>(Bs) + lane;
#pragma unroll
        for (int dh = 0; dh < 4; ++dh) {
#pragma unroll
            for (int dw = 0; dw < 4; ++dw) {
                const float* a0p = a_base + (dh * SD_C + dw) * SD_PS;
#pragma unroll
                for (int m4 = 0; m4 < 4; ++m4) {
                    const f32x4 b = b_base[((dh * 4 + dw) * 4 + m4) * 64];
                    const f32x4 a0 = ld4(a0p + 4 * m4);
                    const f32x4 a1 = ld4(a0p + SD_C * SD_PS + 4 * m4);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[c], b[c], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[c], b[c], acc1, 0, 0, 0);
                    }
                }
            }
        }
        // acc[r] = D[site 4 q + r][n = p]  ->  Os[(site row * 2 + ph) * 3 + ci][2 site + pw]
        if (p < 12) {
            const int cls = p / 3, ci = p - 3 * cls, ph = cls >> 1, pw = cls & 1;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                Os[((0 * 2 + ph) * 3 + ci) * 32 + 2 * (4 * q + r) + pw] = acc0[r];
                Os[((1 * 2 + ph) * 3 + ci) * 32 + 2 * (4 * q + r) + pw] = acc1[r];
            }
        }
        __builtin_amdgcn_wave_barrier();         // Os is the wave's own: its LDS operations complete in order
        const int tj = (int)(t % nTj), ti = (int)((t / nTj) % nTi), img = (int)(t / ((long long)nTj * nTi));
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int idx = k * 64 + lane;
            const int col = idx & 31, row = idx >> 5;            // row = (site row * 2 + ph) * 3 + ci
            const int ci = row % 3, hh = row / 3;                // hh = 2 * site row + ph
            const int h = 2 * (ti * SD_TI + 2 * wave) + hh, wc = 2 * tj * SD_TJ + col;
            if (h < H && wc < W) {
                const size_t o = NHWC_OUT ? (((size_t)img * H + h) * W + wc) * 3 + ci : (((size_t)img * 3 + ci) * H + h) * W + wc;
                dx[o] = Os[idx];
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// EfficientNet-B0 stem: y[oh][ow][co] = sum w[co][kh][kw][ci] x[2 oh + kh - pt][2 ow + kw - pl][ci]; one thread per input pixel.
// Weights in LDS as [kh][kw][ci][32 co]; every lane of a wave reads the same address (broadcast).
template <typename T, bool NHWC_OUT>
__global__ __launch_bounds__(256) void eff_stem_dgrad_kernel(const T* __restrict__ dy, const float* __restrict__ w,
                                                             float* __restrict__ dx, int imgs, int H, int W, int Ho, int Wo,
                                                             int pt, int pl, int Kw, int kw_p, int cin_p)
{
    __shared__ __attribute__((aligned(16))) float ws[9 * 3 * 32];
    for (int e = threadIdx.x; e < 9 * 3 * 32; e += 256) {
        const int co = e & 31, ci = (e >> 5) % 3, tap = e / 96;
        ws[e] = w[(size_t)co * Kw + ((tap / 3) * kw_p + tap % 3) * cin_p + ci];
    }
    __syncthreads();
    const long long npix = (long long)imgs * H * W;
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= npix) return;
    const int wc = (int)(g % W), h = (int)((g / W) % H), img = (int)(g / ((long long)W * H));
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
        const int th = h + pt - kh, oh = th >> 1;
        if (th < 0 || (th & 1) || oh >= Ho) continue;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int tw = wc + pl - kw, ow = tw >> 1;
            if (tw < 0 || (tw & 1) || ow >= Wo) continue;
            const T* src = dy + (((size_t)img * Ho + oh) * Wo + ow) * 32;
            const float* wt = ws + (kh * 3 + kw) * 96;
#pragma unroll
            for (int c4 = 0; c4 < 8; ++c4) {
                const f32x4 d = ld4(src + 4 * c4);
                const f32x4 w0 = ld4(wt + 4 * c4), w1 = ld4(wt + 32 + 4 * c4), w2 = ld4(wt + 64 + 4 * c4);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    a0 = fmaf(d[c], w0[c], a0);
                    a1 = fmaf(d[c], w1[c], a1);
                    a2 = fmaf(d[c], w2[c], a2);
                }
            }
        }
    }
    if (NHWC_OUT) {
        float* o = dx + (size_t)g * 3;
        o[0] = a0; o[1] = a1; o[2] = a2;
    } else {
        const size_t plane = (size_t)H * W, o = (size_t)img * 3 * plane + (size_t)h * W + wc;
        dx[o] = a0; dx[o + plane] = a1; dx[o + 2 * plane] = a2;
    }
}

}  // namespace

size_t stem_dgrad_pack_floats() { return SD_B; }

void k_stem_dgrad_pack(const float* w, float* pack, int Kw, int kw_p, int cin_p, hipStream_t s)
{
    hipLaunchKernelGGL(stem_dgrad_pack_kernel, dim3(SD_B / 256), dim3(256), 0, s, w, pack, Kw, kw_p, cin_p);
}

void k_stem_dgrad(const float* dy, const float* pack, float* dx, int imgs, int Ho, int Wo, int H, int W, int nhwc_out, hipStream_t s)
{
    static bool attr_done = false;
    if (!attr_done) {
        set_max_dyn_lds(reinterpret_cast<const void*>(stem_dgrad_kernel<false>), SD_LDS, "stem_dgrad_kernel");
        set_max_dyn_lds(reinterpret_cast<const void*>(stem_dgrad_kernel<true>), SD_LDS, "stem_dgrad_kernel (NHWC)");
        attr_done = true;
    }
    const long long ntiles = (long long)imgs * ((Ho + SD_TI - 1) / SD_TI) * ((Wo + SD_TJ - 1) / SD_TJ);
    const int grid = (int)(ntiles < 256 ? ntiles : 256);        // one persistent block per CU (122 KB of LDS each)
    if (nhwc_out) hipLaunchKernelGGL(stem_dgrad_kernel<true>, dim3(grid), dim3(256), SD_LDS, s, dy, pack, dx, imgs, Ho, Wo, H, W);
    else hipLaunchKernelGGL(stem_dgrad_kernel<false>, dim3(grid), dim3(256), SD_LDS, s, dy, pack, dx, imgs, Ho, Wo, H, W);
}

void k_eff_stem_dgrad(const void* dy, int dt, const float* w, float* dx, int imgs, int H, int W, int Ho, int Wo, int pad_t,
                      int pad_l, int Kw, int kw_p, int cin_p, int nhwc_out, hipStream_t s)
{
    const long long npix = (long long)imgs * H * W;
    const dim3 grid((unsigned)((npix + 255) / 256)), blk(256);
#define EFF_SD(T, N) hipLaunchKernelGGL((eff_stem_dgrad_kernel<T, N>), grid, blk, 0, s, (const T*)dy, w, dx, imgs, H, W, Ho, Wo, \
                                        pad_t, pad_l, Kw, kw_p, cin_p)
    if (dt == DT_BF16) { if (nhwc_out) EFF_SD(bf16, true); else EFF_SD(bf16, false); }
    else { if (nhwc_out) EFF_SD(float, true); else EFF_SD(float, false); }
#undef EFF_SD
}

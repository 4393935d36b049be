// The FixMatch strong view on the HBM-resident uint8 cache (dataset/dataset.py:63-77):
//   weak affine + flip (as augment_kernel) -> RandAugmentMC(n=2, m=10) (utils/FixMatch.py:205-219) -> CutoutAbs(16) -> /255 -> normalise
// bit-exact with Pillow 12.2 on uint8 images (tests/golden/augment_strong_pil.npz).  The draws are the host's
// (fedmlp_amd/augment.py draw_strong); the record layout is documented at fm_augment_strong in include/fedmlp_hip.h.
//
// Five launches per call, whatever B and whatever ops were drawn; the op of a sample is uniform per workgroup (blockIdx.y = sample):
//   1. strong_weak_kernel        cache -> A   the weak view as uint8
//   2. strong_stats_kernel<0>    A -> stats   per-image histograms -> AutoContrast / Equalize LUT, Contrast mean (only where slot 0 asks)
//   3. strong_apply_kernel       A -> B       op of slot 0 (a copy for Identity / a skipped slot)
//   4. strong_stats_kernel<1>    B -> stats   the same for slot 1, on the image slot 0 produced (fill zeros of a geometric op included)
//   5. strong_final_kernel       B -> out     op of slot 1, cutout, /255, normalise, fp32 NCHW
// A and B are uint8 [max_images][3][H][W] workspaces of the handle (2 x 147 KB per 224^2 image: L2 / Infinity Cache resident).
// Every op reads its source image and writes another buffer, so the gathers (geometric ops, Sharpness' 3x3) never see their own output.
//
// Pillow's arithmetic, restated:
//   ImageEnhance.* = Image.blend(degenerate, image, f), libImaging/Blend.c for 0 <= f <= 1:
//       (UINT8)((int)d + f * ((int)x - (int)d)), f a C float, product and sum rounded separately (no FMA), the cast truncating.
//     Brightness: d = 0.  Color: d = L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 (libImaging/Convert.c).
//     Contrast: d = int(mean(L) + 0.5), a double mean over the image (ImageStat).  Sharpness: d = ImageFilter.SMOOTH, the 3x3 kernel
//     (1,1,1,1,5,1,1,1,1)/13 of libImaging/Filter.c with the border row / column copied.  Filter.c sums fp32 products and truncates
//     after + 0.5; the exact value is T/13 + 0.5 with T an integer, never closer than 1/26 to an integer, so the fp32 rounding cannot
//     change the truncation and (2 T + 13) / 26 in integers is the same byte.
//   ImageOps.autocontrast / equalize: per-channel 256-bin histogram -> LUT (ImageOps.py; autocontrast in doubles, rounded separately).
//   ImageOps.posterize: x & mask.  ImageOps.solarize: x < threshold ? x : 255 - x.
//   Image.rotate / Image.transform(AFFINE) with NEAREST: the 16.16 fixed-point walk of libImaging/Geometry.c, as augment_kernel.
//   ImageDraw.rectangle(xy, (127,127,127)): both corners inclusive.
#include "common.h"
#include "kernels.h"

// Pillow's C rounds a product before it adds to it.  The compiler's default contraction would fuse the two into one FMA, and so
// it does through __fmul_rn / __fadd_rn, which are a plain `*` and `+` inside this toolchain's headers, out of this pragma's reach
// (measured: 68 bytes of fixture case 4 off by one).  So contraction is off for this file and the blend and the AutoContrast table
// are written with the operators themselves.  (The IEEE division keeps the fma instructions of its own expansion: that is the
// correctly rounded quotient, not a contraction.)
#pragma clang fp contract(off)

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

namespace {

enum : int {
    OP_AUTOCONTRAST = 0, OP_BRIGHTNESS, OP_COLOR, OP_CONTRAST, OP_EQUALIZE, OP_IDENTITY, OP_POSTERIZE, OP_ROTATE, OP_SHARPNESS,
    OP_SHEARX, OP_SHEARY, OP_SOLARIZE, OP_TRANSLATEX, OP_TRANSLATEY, OP_SKIP
};
constexpr int REC = FM_STRONG_RECORD;             // int32 per sample: two slots of 8, then the cutout corners
constexpr int STAT = FM_STRONG_STAT_BYTES;        // per sample: 3 x 256 LUT bytes, then the Contrast mean (int32)

__device__ __forceinline__ bool op_is_geometric(int op)
{
    return op == OP_ROTATE || op == OP_SHEARX || op == OP_SHEARY || op == OP_TRANSLATEX || op == OP_TRANSLATEY;
}

__device__ __forceinline__ int blend8(int d, int x, float f)
{
    const float t = f * (float)(x - d);                 // rounded here ...
    return (int)((float)d + t);                         // ... and again here
}

__device__ __forceinline__ int smooth8(const uint8_t* __restrict__ p, int W)
{
    const int t = p[-W - 1] + p[-W] + p[-W + 1] + p[-1] + 5 * p[0] + p[1] + p[W - 1] + p[W] + p[W + 1];
    return (2 * t + 13) / 26;
}

// One pixel (x, y) of `op` applied to the image src[3][H][W].  sl = the slot's 8 int32, st = the sample's LUT / mean.  `op` and
// everything read through sl / st are uniform over the workgroup.
__device__ __forceinline__ void op_pixel(const uint8_t* __restrict__ src, const int* __restrict__ sl, const uint8_t* __restrict__ st,
                                         int op, int x, int y, int H, int W, int& r, int& g, int& b)
{
    const int HW = H * W;
    if (op_is_geometric(op)) {
        const int xin = (sl[3] + sl[1] * x + sl[2] * y) >> 16;
        const int yin = (sl[6] + sl[4] * x + sl[5] * y) >> 16;
        const bool ok = xin >= 0 && xin < W && yin >= 0 && yin < H;
        const uint8_t* p = src + (ok ? yin * W + xin : 0);
        r = ok ? p[0] : 0; g = ok ? p[HW] : 0; b = ok ? p[2 * HW] : 0;
        return;
    }
    const uint8_t* p = src + y * W + x;
    r = p[0]; g = p[HW]; b = p[2 * HW];
    const float f = __int_as_float(sl[1]);
    switch (op) {
    case OP_AUTOCONTRAST:
    case OP_EQUALIZE: r = st[r]; g = st[256 + g]; b = st[512 + b]; break;
    case OP_BRIGHTNESS: r = blend8(0, r, f); g = blend8(0, g, f); b = blend8(0, b, f); break;
    case OP_COLOR: {
        const int L = (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16;
        r = blend8(L, r, f); g = blend8(L, g, f); b = blend8(L, b, f);
    } break;
    case OP_CONTRAST: {
        const int m = *reinterpret_cast<const int*>(st + 768);
        r = blend8(m, r, f); g = blend8(m, g, f); b = blend8(m, b, f);
    } break;
    case OP_SHARPNESS:
        if (x > 0 && x < W - 1 && y > 0 && y < H - 1) {
            r = blend8(smooth8(p, W), r, f); g = blend8(smooth8(p + HW, W), g, f); b = blend8(smooth8(p + 2 * HW, W), b, f);
        }
        break;
    case OP_POSTERIZE: r &= sl[1]; g &= sl[1]; b &= sl[1]; break;
    case OP_SOLARIZE: r = r < sl[1] ? r : 255 - r; g = g < sl[1] ? g : 255 - g; b = b < sl[1] ? b : 255 - b; break;
    default: break;                                     // Identity, a skipped slot
    }
}

// four pixels x..x+3 of row y per thread (W % 4 == 0), one 32-bit store per channel plane
__global__ void strong_weak_kernel(const uint8_t* __restrict__ cache, const int* __restrict__ idx, const int* __restrict__ params,
                                   uint8_t* __restrict__ A, int H, int W)
{
    const int b = blockIdx.y, HW = H * W;
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= HW) return;
    const int y = i / W, x0 = i - y * W;
    const int* p = params + b * 8;
    const uint8_t* src = cache + (size_t)idx[b] * 3 * HW;
    uint32_t o0 = 0, o1 = 0, o2 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = x0 + k;
        const int xs = p[6] != 0 ? W - 1 - x : x;
        const int xin = (p[2] + p[0] * xs + p[1] * y) >> 16;
        const int yin = (p[5] + p[3] * xs + p[4] * y) >> 16;
        const bool ok = xin >= 0 && xin < W && yin >= 0 && yin < H;
        const uint8_t* q = src + (ok ? yin * W + xin : 0);
        o0 |= (ok ? (uint32_t)q[0] : 0u) << (8 * k);
        o1 |= (ok ? (uint32_t)q[HW] : 0u) << (8 * k);
        o2 |= (ok ? (uint32_t)q[2 * HW] : 0u) << (8 * k);
    }
    uint8_t* o = A + (size_t)b * 3 * HW + i;
    *reinterpret_cast<uint32_t*>(o) = o0;
    *reinterpret_cast<uint32_t*>(o + HW) = o1;
    *reinterpret_cast<uint32_t*>(o + 2 * HW) = o2;
}

// One workgroup per image.  Integer LDS atomics only, so the result does not depend on the order of arrival.
template <int SLOT>
__global__ __launch_bounds__(1024) void strong_stats_kernel(const uint8_t* __restrict__ img, const int* __restrict__ strong,
                                                            uint8_t* __restrict__ stats, int H, int W)
{
    const int b = blockIdx.x, HW = H * W, n4 = HW / 4, t = threadIdx.x;
    const int op = strong[b * REC + 8 * SLOT];
    if (op != OP_AUTOCONTRAST && op != OP_EQUALIZE && op != OP_CONTRAST) return;
    __shared__ unsigned hist[768];
    __shared__ unsigned lsum;
    __shared__ int lo[3], hi[3];
    const uint32_t* src = reinterpret_cast<const uint32_t*>(img + (size_t)b * 3 * HW);
    uint8_t* st = stats + (size_t)b * STAT;
    if (op == OP_CONTRAST) {
        if (t == 0) lsum = 0;
        __syncthreads();
        unsigned acc = 0;
        for (int i = t; i < n4; i += blockDim.x) {
            const uint32_t r = src[i], g = src[n4 + i], bl = src[2 * n4 + i];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                acc += (19595u * ((r >> (8 * k)) & 255u) + 38470u * ((g >> (8 * k)) & 255u) + 7471u * ((bl >> (8 * k)) & 255u) + 0x8000u) >> 16;
        }
        atomicAdd(&lsum, acc);                           // <= 255 * H * W: fits 32 bits up to 16 M pixels
        __syncthreads();
        // ImageStat mean = sum / count in doubles; ImageEnhance.Contrast takes int(mean + 0.5)
        if (t == 0) *reinterpret_cast<int*>(st + 768) = (int)((double)lsum / (double)HW + 0.5);
        return;
    }
    if (t < 768) hist[t] = 0;
    if (t < 3) { lo[t] = 255; hi[t] = 0; }
    __syncthreads();
    for (int i = t; i < 3 * n4; i += blockDim.x) {
        const uint32_t w = src[i];
        unsigned* h = hist + 256 * (i / n4);
        atomicAdd(&h[w & 255u], 1u); atomicAdd(&h[(w >> 8) & 255u], 1u); atomicAdd(&h[(w >> 16) & 255u], 1u); atomicAdd(&h[w >> 24], 1u);
    }
    __syncthreads();
    if (t < 768 && hist[t] != 0) { atomicMin(&lo[t >> 8], t & 255); atomicMax(&hi[t >> 8], t & 255); }
    __syncthreads();
    if (t >= 768) return;
    const int c = t >> 8, ix = t & 255, l = lo[c], h = hi[c];
    int v = ix;
    if (op == OP_AUTOCONTRAST) {
        if (h > l) {                                     // scale = 255.0 / (hi - lo); offset = -lo * scale; int(ix * scale + offset)
            const double scale = 255.0 / (double)(h - l);
            const double offset = -(double)l * scale;
            const double prod = (double)ix * scale;
            v = (int)(prod + offset);
            v = v < 0 ? 0 : (v > 255 ? 255 : v);
        }
    } else {                                             // step = (sum(h) - last non-zero bin) // 255; lut[i] = (step // 2 + sum(h[:i])) // step
        const unsigned step = ((unsigned)HW - hist[256 * c + h]) / 255u;
        if (step != 0) {
            unsigned n = step / 2;
            for (int j = 0; j < ix; ++j) n += hist[256 * c + j];
            n /= step;
            v = n > 255u ? 255 : (int)n;                 // Image.point clips the table to 8 bits
        }
    }
    st[t] = (uint8_t)v;
}

__global__ void strong_apply_kernel(const uint8_t* __restrict__ A, const int* __restrict__ strong, const uint8_t* __restrict__ stats,
                                    uint8_t* __restrict__ Bo, int H, int W)
{
    const int b = blockIdx.y, HW = H * W;
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= HW) return;
    const int y = i / W, x0 = i - y * W;
    const int* sl = strong + b * REC;
    const int op = sl[0];
    const uint8_t* src = A + (size_t)b * 3 * HW;
    const uint8_t* st = stats + (size_t)b * STAT;
    uint32_t o0 = 0, o1 = 0, o2 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int r, g, bl;
        op_pixel(src, sl, st, op, x0 + k, y, H, W, r, g, bl);
        o0 |= (uint32_t)r << (8 * k); o1 |= (uint32_t)g << (8 * k); o2 |= (uint32_t)bl << (8 * k);
    }
    uint8_t* o = Bo + (size_t)b * 3 * HW + i;
    *reinterpret_cast<uint32_t*>(o) = o0;
    *reinterpret_cast<uint32_t*>(o + HW) = o1;
    *reinterpret_cast<uint32_t*>(o + 2 * HW) = o2;
}

__global__ void strong_final_kernel(const uint8_t* __restrict__ Bi, const int* __restrict__ strong, const uint8_t* __restrict__ stats,
                                    float* __restrict__ out, int H, int W, float m0, float m1, float m2, float s0, float s1, float s2)
{
    const int b = blockIdx.y, HW = H * W;
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= HW) return;
    const int y = i / W, x0 = i - y * W;
    const int* sl = strong + b * REC + 8;
    const int* cut = strong + b * REC + 16;
    const int op = sl[0];
    const uint8_t* src = Bi + (size_t)b * 3 * HW;
    const uint8_t* st = stats + (size_t)b * STAT;
    const bool yin = y >= cut[1] && y <= cut[3];
    f32x4 o0, o1, o2;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int r, g, bl;
        op_pixel(src, sl, st, op, x0 + k, y, H, W, r, g, bl);
        if (yin && x0 + k >= cut[0] && x0 + k <= cut[2]) r = g = bl = 127;
        // ToTensor: float32 / 255 ; Normalize: (v - mean) / std -- IEEE division, no reciprocal, no contraction (as augment_kernel)
        o0[k] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)r, 255.f), m0), s0);
        o1[k] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)g, 255.f), m1), s1);
        o2[k] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)bl, 255.f), m2), s2);
    }
    float* o = out + (size_t)b * 3 * HW + i;
    *reinterpret_cast<f32x4*>(o) = o0;
    *reinterpret_cast<f32x4*>(o + HW) = o1;
    *reinterpret_cast<f32x4*>(o + 2 * HW) = o2;
}

}  // namespace

void k_augment_strong(const uint8_t* cache, const int* idx, const int* params, const int* strong, uint8_t* ws, int maxB,
                      float* out, int B, int H, int W, float m0, float m1, float m2, float s0, float s1, float s2, hipStream_t s)
{
    const size_t img = (size_t)3 * H * W;
    uint8_t *A = ws, *Bb = ws + (size_t)maxB * img, *stats = ws + 2 * (size_t)maxB * img;
    const dim3 grid(cdiv((int64_t)H * W / 4, 256), B), blk(256);
    hipLaunchKernelGGL(strong_weak_kernel, grid, blk, 0, s, cache, idx, params, A, H, W);
    hipLaunchKernelGGL(strong_stats_kernel<0>, dim3(B), dim3(1024), 0, s, A, strong, stats, H, W);
    hipLaunchKernelGGL(strong_apply_kernel, grid, blk, 0, s, A, strong, stats, Bb, H, W);
    hipLaunchKernelGGL(strong_stats_kernel<1>, dim3(B), dim3(1024), 0, s, Bb, strong, stats, H, W);
    hipLaunchKernelGGL(strong_final_kernel, grid, blk, 0, s, Bb, strong, stats, out, H, W, m0, m1, m2, s0, s1, s2);
}

// Pre/post-processing and glue kernels of the hot path: preprocess, context conv 1->128, EgoLanes feature fusion,
// decode, output resizes, layout conversions.  (Encoder pieces: kernels_backbone.hip; convs: kernels_conv*.hip.)
#include "act_io.hpp"

namespace vp {

// ------------------------------------------------------------------------------------------ preprocess
// Integer bilinear (definition: oracle/pre_post.py resize_bilinear_u8; modelled on cv::resize INTER_LINEAR,
// onnx_runtime_backend.cpp:44) + /255 + (x-mean)/std + HWC->CHW (onnx_runtime_backend.cpp:45-57,
// onnxruntime_engine.cpp:72-102).  Tap tables are built on the host so the device does integer math only.
// The u8 -> [0, 1] step exists in two spellings that differ in the last bit for 322 of the 768 (byte, channel) pairs:
//   norm_form 0  q / 255            torchvision to_tensor (Models/inference/scene_seg_infer.py:15-20): one IEEE division
//   norm_form 1  q * fl(1 / 255)    cv::Mat::convertTo(CV_32FC3, 1.0 / 255.0) of the C++ front-ends (onnx_runtime_backend.cpp:45,
//                                   tensorrt_backend.cpp:164, onnxruntime_engine.cpp:85): the scale is rounded to float once, then multiplied
// followed in both by the float subtraction and the IEEE float division the sources spell out (cv::subtract / cv::divide by a Scalar
// converted to float, :48-49; the scalar loop (x - MEAN[c]) / STD[c], onnxruntime_engine.cpp:98).
__device__ __forceinline__ float unit_from_u8(int q, int norm_form) {
  return norm_form ? __fmul_rn((float)q, (float)(1.0 / 255.0)) : __fdiv_rn((float)q, 255.0f);
}
// byte `sc` of one resized pixel: r0 / r1 the two source rows of yt, xt / yt one entry of the tap tables (linear_taps_u8).  Shared with canvas_resize_kernel.
__device__ __forceinline__ int bilinear_u8(const uint8_t* r0, const uint8_t* r1, const int4& xt, const int4& yt, int sc) {
  const int s0 = (int)r0[xt.x * 3 + sc] * xt.z + (int)r0[xt.y * 3 + sc] * xt.w;
  const int s1 = (int)r1[xt.x * 3 + sc] * xt.z + (int)r1[xt.y * 3 + sc] * xt.w;
  const int q = (((yt.z * (s0 >> 4)) >> 16) + ((yt.w * (s1 >> 4)) >> 16) + 2) >> 2;
  return min(max(q, 0), 255);
}
__global__ __launch_bounds__(256) void preprocess_kernel(const PreprocessParams p) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= p.out_w) return;
  const int4 xt = *reinterpret_cast<const int4*>(p.xtab + 4 * x);
  const int4 yt = *reinterpret_cast<const int4*>(p.ytab + 4 * y);
  const uint8_t* r0 = p.frame + (size_t)yt.x * p.stride;
  const uint8_t* r1 = p.frame + (size_t)yt.y * p.stride;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int q = bilinear_u8(r0, r1, xt, yt, p.src_c[c]);
    const float t = unit_from_u8(q, p.norm_form);
    p.out[((size_t)c * p.out_h + y) * p.out_w + x] = __fdiv_rn(__fsub_rn(t, p.mean[c]), p.stdv[c]);
  }
}

// ------------------------------------------------------------------------------------------ vp_frame: native camera formats -> BGR8
// One work-item produces four pixels of a row (the 4:2:0 formats: of two rows, i.e. two whole 2x2 chroma groups; YUY2 / UYVY: two 2x1 groups), so every
// chroma sample is read once, and stores them as three aligned 32-bit words per row (kernels.hpp FrameToBgrParams: rows are 12 * ceil(w / 4) bytes apart).
// Pixels beyond the row's end are written as zero bytes.  Source planes are read byte by byte: a decoder surface or a caller's view promises no alignment.
// The YUV formats use the 20-bit integer form include/vp_hip.h states as the DEFINITION, no chroma interpolation; its constants p.k are those of the
// frame's colour standard (kernels.hpp color_standard), uniform over the launch.  The default, BT.601 limited range, is the form documented for OpenCV's
// cvtColor(COLOR_YUV2BGR_NV12 / _YUY2 / _UYVY) (parity with OpenCV itself is not pinned):
//   y = cy * max(0, Y - off), u = U - 128, v = V - 128
//   R = sat8((y + cvr v + 2^19) >> 20), G = sat8((y - cvg v - cug u + 2^19) >> 20), B = sat8((y + cub u + 2^19) >> 20)
struct ChromaTerms {
  int r, g, b;   // the chroma part of each channel, rounding constant included
};
__device__ __forceinline__ ChromaTerms chroma_terms(const YuvToBgr& k, int U, int V) {
  const int u = U - 128, v = V - 128;
  return {k.cvr * v + (1 << 19), -k.cvg * v - k.cug * u + (1 << 19), k.cub * u + (1 << 19)};
}
__device__ __forceinline__ unsigned sat8(int x) { return (unsigned)min(max(x, 0), 255); }
// one pixel as b | g << 8 | r << 16
__device__ __forceinline__ unsigned yuv_pixel(const YuvToBgr& k, int Y, const ChromaTerms& c) {
  const int y = k.cy * max(0, Y - k.off);
  return sat8((y + c.b) >> 20) | (sat8((y + c.g) >> 20) << 8) | (sat8((y + c.r) >> 20) << 16);
}
__device__ __forceinline__ void store_bgr4(uint8_t* row, int j, const unsigned px[4]) {
  uint32_t* d = reinterpret_cast<uint32_t*>(row + 12 * (size_t)j);
  d[0] = px[0] | (px[1] << 24);
  d[1] = (px[1] >> 8) | (px[2] << 16);
  d[2] = (px[2] >> 16) | (px[3] << 8);
}
__global__ __launch_bounds__(256) void frame_to_bgr8_kernel(const FrameToBgrParams p) {
  const int bpr = (p.w + 3) >> 2;                          // four-pixel blocks per row
  const bool f420 = p.format == 5 || p.format >= 16;       // NV12, I420 (YV12 arrives as I420), NV21
  const int rows = f420 ? p.h >> 1 : p.h;                  // 4:2:0: row pairs
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)rows * bpr) return;
  const int r = (int)(t / bpr), j = (int)(t - (long long)r * bpr), x0 = 4 * j;
  unsigned px[4] = {0u, 0u, 0u, 0u};
  if (f420) {   // Y rows 2r, 2r + 1; one (U, V) per 2x2 block.  The formats differ only in where a group's two chroma bytes lie:
    const uint8_t* y0 = p.p0 + (size_t)(2 * r) * p.s0 + x0;
    const uint8_t* y1 = y0 + p.s0;
    const bool planar = p.format == 16;                    // I420: U from p1, V from p2, one byte a group; NV12 / NV21: U V / V U pairs in p1
    const int step = planar ? 1 : 2;
    const uint8_t* cu = p.p1 + (size_t)r * p.s1 + (planar ? x0 >> 1 : x0 + (p.format == 18 ? 1 : 0));
    const uint8_t* cv = planar ? p.p2 + (size_t)r * p.s2 + (x0 >> 1) : p.p1 + (size_t)r * p.s1 + x0 + (p.format == 18 ? 0 : 1);
    unsigned px1[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      if (x0 + 2 * g >= p.w) break;                        // w is even: a group is whole or absent
      const ChromaTerms c = chroma_terms(p.k, cu[step * g], cv[step * g]);
      px[2 * g] = yuv_pixel(p.k, y0[2 * g], c);
      px[2 * g + 1] = yuv_pixel(p.k, y0[2 * g + 1], c);
      px1[2 * g] = yuv_pixel(p.k, y1[2 * g], c);
      px1[2 * g + 1] = yuv_pixel(p.k, y1[2 * g + 1], c);
    }
    store_bgr4(p.dst + (size_t)(2 * r) * p.dst_pitch, j, px);
    store_bgr4(p.dst + (size_t)(2 * r + 1) * p.dst_pitch, j, px1);
    return;
  }
  const uint8_t* row = p.p0 + (size_t)r * p.s0;
  if (p.format >= 6) {   // YUY2: Y0 U Y1 V; UYVY: U Y0 V Y1 -- one (U, V) per horizontal pixel pair
    const int yo = p.format == 6 ? 0 : 1, co = 1 - yo;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      if (x0 + 2 * g >= p.w) break;
      const uint8_t* s = row + 2 * (size_t)(x0 + 2 * g);
      const ChromaTerms c = chroma_terms(p.k, s[co], s[co + 2]);
      px[2 * g] = yuv_pixel(p.k, s[yo], c);
      px[2 * g + 1] = yuv_pixel(p.k, s[yo + 2], c);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int x = x0 + i;
      if (x >= p.w) break;
      if (p.format == 4) {          // GRAY8 replicated
        px[i] = 0x010101u * row[x];
      } else {
        const uint8_t* s = row + (size_t)x * (p.format <= 1 ? 3 : 4);
        const bool rgb = p.format == 1 || p.format == 3;   // RGB8 / RGBA8: R first; BGR8 / BGRA8: B first; alpha dropped
        px[i] = (unsigned)s[rgb ? 2 : 0] | ((unsigned)s[1] << 8) | ((unsigned)s[rgb ? 0 : 2] << 16);
      }
    }
  }
  store_bgr4(p.dst + (size_t)r * p.dst_pitch, j, px);
}

// vp_frame's rectification passes (kernels.hpp FrameRemapParams): a gather through a map of 1/32-pixel source coordinates plus one integer blend per
// channel, the blocks and the store of frame_to_bgr8_kernel.  The four weights sum to 1024, so (sum + 512) >> 10 stays inside 0 .. 255: no clamp.  Each
// channel's value is held in a register of its own before the pixel is packed (see chroma_of below for what a packed shift once did on the device).
__device__ __forceinline__ unsigned own_register(unsigned v) {
  asm volatile("" : "+v"(v));
  return v;
}
__device__ __forceinline__ unsigned remap_pixel(const FrameRemapParams& p, int X, int Y) {
  const int ix = X >> 5, iy = Y >> 5, fx = X & 31, fy = Y & 31;
  const int x0 = min(max(ix, 0), p.src_w - 1), x1 = min(max(ix + 1, 0), p.src_w - 1);
  const int y0 = min(max(iy, 0), p.src_h - 1), y1 = min(max(iy + 1, 0), p.src_h - 1);
  int wx0 = 32 - fx, wx1 = fx, wy0 = 32 - fy, wy1 = fy;
  if (p.border == 0) {   // CONSTANT: a tap the clamp moved lies outside the source and counts as 0
    wx0 = x0 == ix ? wx0 : 0;
    wx1 = x1 == ix + 1 ? wx1 : 0;
    wy0 = y0 == iy ? wy0 : 0;
    wy1 = y1 == iy + 1 ? wy1 : 0;
  }
  const unsigned w00 = (unsigned)(wx0 * wy0), w01 = (unsigned)(wx1 * wy0), w10 = (unsigned)(wx0 * wy1), w11 = (unsigned)(wx1 * wy1);
  const uint8_t* r0 = p.src + (size_t)y0 * p.src_pitch;
  const uint8_t* r1 = p.src + (size_t)y1 * p.src_pitch;
  const uint8_t *a = r0 + 3 * x0, *b = r0 + 3 * x1, *c = r1 + 3 * x0, *d = r1 + 3 * x1;
  const unsigned c0 = (w00 * a[0] + w01 * b[0] + w10 * c[0] + w11 * d[0] + 512u) >> 10;
  const unsigned c1 = own_register((w00 * a[1] + w01 * b[1] + w10 * c[1] + w11 * d[1] + 512u) >> 10);
  const unsigned c2 = own_register((w00 * a[2] + w01 * b[2] + w10 * c[2] + w11 * d[2] + 512u) >> 10);
  return c0 | (c1 << 8) | (c2 << 16);
}
__global__ __launch_bounds__(256) void frame_remap_kernel(const FrameRemapParams p) {
  const int j = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (j >= (p.out_w + 3) >> 2) return;
  const int4* m = reinterpret_cast<const int4*>(p.map + (size_t)y * p.map_pitch + 4 * (size_t)j);
  const int4 m01 = m[0], m23 = m[1];
  const int X[4] = {m01.x, m01.z, m23.x, m23.z}, Y[4] = {m01.y, m01.w, m23.y, m23.w};
  unsigned px[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (4 * j + k >= p.out_w) break;
    px[k] = remap_pixel(p, X[k], Y[k]);
  }
  store_bgr4(p.dst + (size_t)y * p.dst_pitch, j, px);
}

// vp_frame's 16-bit formats (kernels.hpp FrameDeepParams): P010 with NV12's work-item (four pixels of two rows, two whole chroma groups), GRAY16 with
// GRAY8's (four pixels of a row).  Every sample is one aligned 16-bit load, narrowed to x8 = min(255, (s + 128) >> 8) before anything else, so the
// arithmetic behind it is frame_to_bgr8_kernel's to the bit.  The narrowed byte is held in a register of its own (chroma_of: a packed shift-and-clamp).
__device__ __forceinline__ int narrow16(const uint8_t* s) {
  return (int)own_register(min(255u, ((unsigned)*reinterpret_cast<const uint16_t*>(s) + 128u) >> 8));
}
__global__ __launch_bounds__(256) void frame_deep_to_bgr8_kernel(const FrameDeepParams p) {
  const int bpr = (p.w + 3) >> 2;
  const bool p010 = p.format == 21;
  const int rows = p010 ? p.h >> 1 : p.h;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)rows * bpr) return;
  const int r = (int)(t / bpr), j = (int)(t - (long long)r * bpr), x0 = 4 * j;
  unsigned px[4] = {0u, 0u, 0u, 0u};
  if (p010) {   // Y rows 2r, 2r + 1; row r of the U V plane: the words U, V of the group at pixel x lie 2 x bytes in
    const uint8_t* y0 = p.p0 + (size_t)(2 * r) * p.s0 + 2 * (size_t)x0;
    const uint8_t* y1 = y0 + p.s0;
    const uint8_t* uv = p.p1 + (size_t)r * p.s1 + 2 * (size_t)x0;
    unsigned px1[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      if (x0 + 2 * g >= p.w) break;                        // w is even: a group is whole or absent
      const ChromaTerms c = chroma_terms(p.k, narrow16(uv + 4 * g), narrow16(uv + 4 * g + 2));
      px[2 * g] = yuv_pixel(p.k, narrow16(y0 + 4 * g), c);
      px[2 * g + 1] = yuv_pixel(p.k, narrow16(y0 + 4 * g + 2), c);
      px1[2 * g] = yuv_pixel(p.k, narrow16(y1 + 4 * g), c);
      px1[2 * g + 1] = yuv_pixel(p.k, narrow16(y1 + 4 * g + 2), c);
    }
    store_bgr4(p.dst + (size_t)(2 * r) * p.dst_pitch, j, px);
    store_bgr4(p.dst + (size_t)(2 * r + 1) * p.dst_pitch, j, px1);
    return;
  }
  const uint8_t* row = p.p0 + (size_t)r * p.s0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (x0 + i >= p.w) break;
    px[i] = 0x010101u * (unsigned)narrow16(row + 2 * (size_t)(x0 + i));
  }
  store_bgr4(p.dst + (size_t)r * p.dst_pitch, j, px);
}

// vp_frame's raw Bayer formats (kernels.hpp FrameRawParams; include/vp_hip.h states the arithmetic as the DEFINITION).  One work-item owns the 4 x 2
// block at (4 j, 2 r) -- two whole CFA cells, two store_bgr4 rows -- and reads its 6 x 4 window once, linearising and white-balancing each sample as it
// arrives.  Window position (wy, wx) is the site (2 r - 1 + wy, 4 j - 1 + wx), so its CFA colour depends on (wy, wx) and the two uniform order bits only:
// every colour decision below is uniform over the launch.  16-bit samples are aligned 16-bit loads, 8-bit samples bytes.  No LDS, no atomics.
__device__ __forceinline__ int mirror_index(int i, int n) {   // -1 -> 1, n -> n - 2; the clamp only meets columns that no pixel inside the row reads
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * n - 2 - i : i;
  return min(max(i, 0), n - 1);
}
__device__ __forceinline__ int raw_matrix_row(const int* k, int r, int g, int b, int M) { return min(max((k[0] * r + k[1] * g + k[2] * b + 512) >> 10, 0), M); }
__global__ __launch_bounds__(256) void frame_raw_to_bgr8_kernel(const FrameRawParams p) {
  const int bpr = (p.w + 3) >> 2;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)(p.h >> 1) * bpr) return;
  const int r = (int)(t / bpr), j = (int)(t - (long long)r * bpr), x0 = 4 * j, y0 = 2 * r;
  const int M = (1 << p.bits) - 1;
  int cx[6];
#pragma unroll
  for (int wx = 0; wx < 6; ++wx) cx[wx] = mirror_index(x0 - 1 + wx, p.w);
  int v[4][6];
#pragma unroll
  for (int wy = 0; wy < 4; ++wy) {
    const uint8_t* row = p.src + (size_t)mirror_index(y0 - 1 + wy, p.h) * p.stride;
    const int yodd = (wy + 1) & 1;                         // y0 is even
#pragma unroll
    for (int wx = 0; wx < 6; ++wx) {
      const int xodd = (wx + 1) & 1;                       // x0 is a multiple of 4
      const int gain = ((xodd ^ yodd ^ p.green00) & 1) ? p.gains[1] : (yodd != p.red_row0 ? p.gains[0] : p.gains[2]);
      const int s = p.wide ? (int)*reinterpret_cast<const uint16_t*>(row + 2 * (size_t)cx[wx]) : (int)row[cx[wx]];
      const int lin = max(0, min(s >> p.shift, M) - p.black);
      v[wy][wx] = min(M, (lin * gain + 128) >> 8);
    }
  }
  const int lut_shift = p.bits > 12 ? p.bits - 12 : 0;
  const int tone_shift = p.bits - 8, tone_round = p.bits > 8 ? 1 << (p.bits - 9) : 0;
  unsigned px[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
#pragma unroll
  for (int py = 0; py < 2; ++py) {
    const bool red_row = py != p.red_row0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (x0 + k >= p.w) break;
      const int wy = py + 1, wx = k + 1;
      const int c = v[wy][wx], n = v[wy - 1][wx], s = v[wy + 1][wx], w = v[wy][wx - 1], e = v[wy][wx + 1];
      int R, G, B;
      if ((k ^ py ^ p.green00) & 1) {   // a green site: one colour left and right, the other above and below
        const int hor = (w + e + 1) >> 1, ver = (n + s + 1) >> 1;
        G = c;
        R = red_row ? hor : ver;
        B = red_row ? ver : hor;
      } else {                          // a red or blue site: green on the cross, the opposite colour on the diagonals
        const int diag = (v[wy - 1][wx - 1] + v[wy - 1][wx + 1] + v[wy + 1][wx - 1] + v[wy + 1][wx + 1] + 2) >> 2;
        G = (n + s + w + e + 2) >> 2;
        R = red_row ? c : diag;
        B = red_row ? diag : c;
      }
      if (p.ccm_on) {
        const int r2 = raw_matrix_row(p.ccm, R, G, B, M), g2 = raw_matrix_row(p.ccm + 3, R, G, B, M), b2 = raw_matrix_row(p.ccm + 6, R, G, B, M);
        R = r2;
        G = g2;
        B = b2;
      }
      if (p.lut) {
        R = p.lut[R >> lut_shift];
        G = p.lut[G >> lut_shift];
        B = p.lut[B >> lut_shift];
      } else if (p.bits > 8) {
        R = min(255, (R + tone_round) >> tone_shift);
        G = min(255, (G + tone_round) >> tone_shift);
        B = min(255, (B + tone_round) >> tone_shift);
      }
      px[py][k] = own_register((unsigned)B) | (own_register((unsigned)G) << 8) | (own_register((unsigned)R) << 16);   // own registers: see chroma_of
    }
  }
  store_bgr4(p.dst + (size_t)y0 * p.dst_pitch, j, px[0]);
  store_bgr4(p.dst + (size_t)(y0 + 1) * p.dst_pitch, j, px[1]);
}

// Pillow's 8-bit resample passes (kernels.hpp PilResampleParams): int32 accumulation from 1 << 21 of u8 x 22-bit coefficients,
// `>> 22`, clip to u8 (Resample.c clip8) -- integer work, bit-exact by construction.
__device__ __forceinline__ int pil_clip8(int acc) { return min(max(acc >> 22, 0), 255); }
__global__ __launch_bounds__(256) void pil_resample_h_kernel(const PilResampleParams p) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= p.out_w) return;
  const int lo = p.hb[2 * x], n = p.hb[2 * x + 1];
  const int* k = p.hk + (size_t)x * p.hks;
  const uint8_t* row = p.frame + (size_t)y * p.stride + (size_t)lo * 3;
  int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
  for (int t = 0; t < n; ++t) {
    const int kt = k[t];
    a0 += (int)row[3 * t + 0] * kt;
    a1 += (int)row[3 * t + 1] * kt;
    a2 += (int)row[3 * t + 2] * kt;
  }
  uint8_t* d = p.tmp + ((size_t)y * p.out_w + x) * 3;
  d[0] = (uint8_t)pil_clip8(a0);
  d[1] = (uint8_t)pil_clip8(a1);
  d[2] = (uint8_t)pil_clip8(a2);
}
__global__ __launch_bounds__(256) void pil_resample_v_kernel(const PilResampleParams p) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= p.out_w) return;
  const int lo = p.vb[2 * y], n = p.vb[2 * y + 1];
  const int* k = p.vk + (size_t)y * p.vks;
  const uint8_t* col = p.tmp + ((size_t)lo * p.out_w + x) * 3;
  int a[3] = {1 << 21, 1 << 21, 1 << 21};
  for (int t = 0; t < n; ++t) {
    const int kt = k[t];
    const uint8_t* s = col + (size_t)t * p.out_w * 3;
    a[0] += (int)s[0] * kt;
    a[1] += (int)s[1] * kt;
    a[2] += (int)s[2] * kt;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int sc = p.src_c[c];
    const int q = pil_clip8(sc == 0 ? a[0] : (sc == 1 ? a[1] : a[2]));
    const float t = unit_from_u8(q, p.norm_form);   // default 0: torchvision to_tensor, u8 -> fp32 / 255
    p.out[((size_t)c * p.out_h + y) * p.out_w + x] = __fdiv_rn(__fsub_rn(t, p.mean[c]), p.stdv[c]);
  }
}

// context_layer_3: Conv 3x3 1->128 on the 10x20 sigmoid map + GELU (scene_context.py:19,46-47).
__global__ __launch_bounds__(256) void ctx_conv1_kernel(const CtxConv1Params p) {
  const int CG = p.out.C >> 3;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= p.H * p.W * CG) return;
  const int cg = t % CG, pix = t / CG;
  const int y = pix / p.W, x = pix - y * p.W;
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = p.b[cg * 8 + i];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int iy = y + ky - 1, ix = x + kx - 1;
      const float v = ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) ? p.map[iy * p.W + ix] : 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = fmaf(v, p.w[(ky * 3 + kx) * p.out.C + cg * 8 + i], acc[i]);
    }
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = p.act == ACT_GELU ? gelu_exact(acc[i]) : apply_act(acc[i], p.act);
  if (p.scaled) {
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] *= p.out_mul;
  }
  store8(p.out, (size_t)pix * p.out.C + cg * 8, acc);
}

// Round 5: the matvec that builds the one-channel H x W map (scene networks: context_layer_2 + sigmoid; AutoDrive CTX: exp0 + SiLU twice) FUSED with
// the 3x3 convolution 1 -> C that reads it (context_layer_3 / ctx0): the map was a launch boundary and 0.8 - 131 KB through HBM for a tensor a
// workgroup can rebuild where it needs it.  A workgroup owns a T x T pixel patch: (1) x -- the previous layer's vector, or the average pool rebuilt
// from slab partials in their fixed order -- goes to LDS; (2) the (T + 2)^2 map values under the patch: row n of the matrix against x, G lanes per
// row (each a strided quarter-vector walk, then an xor-shuffle tree: a fixed order), bias, activation, zero outside the map (the convolution pads the
// MAP); (3) the nine taps per (pixel, channel octet), ctx_conv1_kernel's arithmetic term for term.  Neighbouring workgroups recompute the halo rows
// (1.27x at T = 16, 1.56x at T = 8: a few thousand multiply-adds).
template <int T>
__global__ __launch_bounds__(256) void ctx_exp_conv1_kernel(const CtxExpConv1Params q) {
  extern __shared__ __attribute__((aligned(16))) float smem_f[];
  const FcParams& p = q.fc;
  const CtxConv1Params& c = q.cv;
  constexpr int HT = T + 2;
  float* const xs = smem_f;                       // [K]
  float* const mp = smem_f + ((p.K + 3) & ~3);    // [HT][HT]
  for (int k = threadIdx.x; k < p.K; k += 256) {
    float xv;
    if (p.partial) {
      xv = 0.f;
#pragma unroll 8
      for (int s = 0; s < p.nslab; ++s) xv += p.partial[(size_t)s * p.Kstride + k];
      xv *= p.inv_hw;
    } else {
      xv = p.x[k];
    }
    xs[k] = xv;
  }
  __syncthreads();
  const int tiles_x = (c.W + T - 1) / T;
  const int y0 = (blockIdx.x / tiles_x) * T, x0 = (blockIdx.x % tiles_x) * T;
  const int G = q.glanes, rows_per_pass = 256 / G;
  const int g = threadIdx.x / G, l = threadIdx.x % G;
  const f32x4_t* x4 = reinterpret_cast<const f32x4_t*>(xs);
  const int K4 = p.K >> 2;
  for (int r0 = 0; r0 < HT * HT; r0 += rows_per_pass) {   // uniform trip count: every lane takes part in the shuffle tree of every pass
    const int r = r0 + g;
    const bool live = r < HT * HT;
    const int hy = r / HT, hx = r - hy * HT;
    const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
    const bool inside = live && (unsigned)iy < (unsigned)c.H && (unsigned)ix < (unsigned)c.W;
    const int n = inside ? iy * c.W + ix : 0;
    float s = 0.f;
    if (p.w8) {
      const unsigned* wr8 = reinterpret_cast<const unsigned*>(p.w8 + (size_t)n * p.K);
#pragma unroll 16
      for (int k = l; k < K4; k += G) {   // (unrolled: a lane's pieces of the row are independent loads -- one or two round trips, not one per piece)
        const unsigned c4 = wr8[k];
        const f32x4_t m = x4[k];
        s += (e4m3_to_float(c4 & 0xffu) * m[0] + e4m3_to_float((c4 >> 8) & 0xffu) * m[1]) + (e4m3_to_float((c4 >> 16) & 0xffu) * m[2] + e4m3_to_float(c4 >> 24) * m[3]);
      }
    } else {
      const f32x4_t* wr = reinterpret_cast<const f32x4_t*>(p.w + (size_t)n * p.K);
#pragma unroll 16
      for (int k = l; k < K4; k += G) {
        const f32x4_t a = wr[k], m = x4[k];
        s += (a[0] * m[0] + a[1] * m[1]) + (a[2] * m[2] + a[3] * m[3]);
      }
    }
    for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (l == 0 && live) mp[r] = inside ? apply_act((p.w8 ? s * p.wscale8[n] : s) + p.b[n], p.act) : 0.f;
  }
  __syncthreads();
  const int CG = c.out.C >> 3;
  for (int t = threadIdx.x; t < T * T * CG; t += 256) {
    const int cg = t % CG, lp = t / CG;
    const int ly = lp / T, lx = lp - ly * T;
    const int y = y0 + ly, x = x0 + lx;
    if (y >= c.H || x >= c.W) continue;
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = c.b[cg * 8 + i];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const float v = mp[(ly + ky) * HT + lx + kx];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = fmaf(v, c.w[(ky * 3 + kx) * c.out.C + cg * 8 + i], acc[i]);
      }
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = c.act == ACT_GELU ? gelu_exact(acc[i]) : apply_act(acc[i], c.act);
    store8(c.out, (size_t)(y * c.W + x) * c.out.C + cg * 8, acc);
  }
}

// --------------------------------------------------------------------------------- EgoLanes feature fusion
// MaxPool2x2 applied n times == max over a 2^n x 2^n window; concat along C (backbone_feature_fusion.py:13-38).
// One thread per output element, walking its window two bytes at a time: the fallback for channel counts that are not octet multiples
// (and, until round 4, the only form: 115 us of an EgoLanes frame -- the 6400 threads of the stride-2 tap each chained 512 loads).
__global__ __launch_bounds__(256) void fusion_kernel(const FusionParams p) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int HW = p.out.H * p.out.W;
  if (t >= HW * p.out.C) return;
  const int c = t % p.out.C, pix = t / p.out.C;
  const int y = pix / p.out.W, x = pix - y * p.out.W;
  float best = 0.0f;
  if (c < p.Creal_out) {
    int lvl = 0, cc = c;
    while (cc >= p.creal[lvl]) { cc -= p.creal[lvl]; ++lvl; }
    const ActView& a = p.f[lvl];
    const int n = 1 << p.shift[lvl];
    best = -3.0e38f;
    for (int dy = 0; dy < n; ++dy)
      for (int dx = 0; dx < n; ++dx) {
        const size_t off = ((size_t)(y * n + dy) * a.W + (x * n + dx)) * a.C + cc;
        float v = (float)a.hi[off];
        if (a.lo) v += (float)a.lo[off];
        best = fmaxf(best, v);
      }
  }
  const half_t h = (half_t)best;
  p.out.hi[t] = h;
  if (p.out.lo) p.out.lo[t] = (half_t)(best - (float)h);
}
// Round 4: one workgroup per output pixel.  A work unit = (tap, channel octet, slice of the tap's window): up to 16 window elements fetched as
// independent 16-byte pieces, their maximum parked in LDS; a second pass takes the maximum over a (tap, octet)'s slices and stores 8 channels.
// Same values as the kernel above (a maximum has no rounding), 16 us instead of 115 (measured).
__global__ __launch_bounds__(256) void fusion_octet_kernel(const FusionParams p) {
  __shared__ float part[512 * 8];
  const int pix = blockIdx.x, tid = threadIdx.x;
  const int y = pix / p.out.W, x = pix - y * p.out.W;
  // unit ranges per tap: octets * slices, slices = min(window elements, 16)
  int ubase[6], nsl[5];
  ubase[0] = 0;
#pragma unroll
  for (int l = 0; l < 5; ++l) {
    const int n2 = 1 << (2 * p.shift[l]);
    nsl[l] = n2 < 16 ? n2 : 16;
    ubase[l + 1] = ubase[l] + (p.creal[l] >> 3) * nsl[l];
  }
  for (int u = tid; u < ubase[5]; u += 256) {
    int l = 0;
    while (u >= ubase[l + 1]) ++l;
    const int r = u - ubase[l], oct = r / nsl[l], sl = r - oct * nsl[l];
    const ActView& a = p.f[l];
    const int n = 1 << p.shift[l], n2 = n * n, per = n2 / nsl[l];
    float best[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) best[i] = -3.0e38f;
#pragma unroll 4
    for (int e = sl * per; e < (sl + 1) * per; ++e) {
      const int dy = e >> p.shift[l], dx = e & (n - 1);
      float v[8];
      load8(a, ((size_t)(y * n + dy) * a.W + (x * n + dx)) * a.C + oct * 8, v);
#pragma unroll
      for (int i = 0; i < 8; ++i) best[i] = fmaxf(best[i], v[i]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) part[u * 8 + i] = best[i];
  }
  __syncthreads();
  const int n_oct = p.out.C >> 3;
  for (int o = tid; o < n_oct; o += 256) {
    float best[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) best[i] = 0.0f;   // pad channels stay zero
    if (o * 8 < p.Creal_out) {
      int l = 0, oc = o;
      while (oc >= (p.creal[l] >> 3)) { oc -= p.creal[l] >> 3; ++l; }
      const float* src = part + (ubase[l] + oc * nsl[l]) * 8;
#pragma unroll
      for (int i = 0; i < 8; ++i) best[i] = src[i];
      for (int s = 1; s < nsl[l]; ++s)
#pragma unroll
        for (int i = 0; i < 8; ++i) best[i] = fmaxf(best[i], src[s * 8 + i]);
    }
    store8(p.out, (size_t)pix * p.out.C + o * 8, best);
  }
}

// ------------------------------------------------------------------------------------------------ decode
// mode 0: argmax over C planes, first max wins, 255 where class==1 (run_model_node.cpp:144-163,
//         cuda_visualization_kernels.cu:13-42); C==1 -> 255 where >0 (:164-171)
// mode 1: lane priority label {2,1,0,255} (cuda_visualization_kernels.cu:45-75)
// mode 2: raw class index (scene_seg_infer.py:52-55)
__global__ __launch_bounds__(256) void decode_mask_kernel(const float* logits, int C, int HW, int mode, uint8_t* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  uint8_t r;
  if (mode == 1) {
    const bool b0 = logits[i] > 0.0f, b1 = logits[HW + i] > 0.0f, b2 = logits[2 * HW + i] > 0.0f;
    r = b2 ? 2 : (b1 ? 1 : (b0 ? 0 : 255));
  } else if (C > 1) {
    float best = -1e9f;
    int cls = 0;
    for (int c = 0; c < C; ++c) {
      const float s = logits[(size_t)c * HW + i];
      if (s > best) { best = s; cls = c; }
    }
    r = mode == 2 ? (uint8_t)cls : (cls == 1 ? 255 : 0);
  } else {
    r = logits[i] > 0.0f ? 255 : 0;
  }
  out[i] = r;
}

// MasksVisualizationEngine::visualize (common/visualizers/masks_visualization_engine.cpp:11-58): colour LUT on the mask
// (createColorMask :41-58; label values not listed stay black), cv::resize INTER_NEAREST to the frame size (:21-25),
// cv::addWeighted(color, 0.5, frame, 0.5, 0) (:29) = saturate_cast<uchar>(cvRound(0.5*a + 0.5*b)): both halves are exact
// in float, cvRound rounds half to even -> (a+b)>>1, plus 1 when the sum is odd and that half is odd.
__device__ __forceinline__ unsigned blend_half_even(unsigned a, unsigned b) {
  const unsigned s2 = a + b, h = s2 >> 1;
  return (s2 & 1) ? h + (h & 1) : h;
}
__global__ __launch_bounds__(256) void viz_blend_kernel(const uint8_t* mask, int mw, const int* ytab, const int* xtab, const uint8_t* frame,
                                                        int stride, int oh, int ow, const uint8_t* lut /* [256][3] BGR */, int frame_is_rgb,
                                                        uint8_t* dst) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= ow) return;
  const uint8_t label = mask[(size_t)ytab[y] * mw + xtab[x]];
  const uint8_t* f = frame + (size_t)y * stride + 3 * x;
  uint8_t* d = dst + ((size_t)y * ow + x) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    d[c] = (uint8_t)blend_half_even(lut[label * 3 + c], f[frame_is_rgb ? 2 - c : c]);
  }
}

// cv::resize INTER_NEAREST (run_model_node.cpp:176-177); index tables from the host.
__global__ __launch_bounds__(256) void resize_nearest_kernel(const uint8_t* src, int sw, const int* ytab, const int* xtab,
                                                             int oh, int ow, uint8_t* dst) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= ow) return;
  dst[(size_t)y * ow + x] = src[(size_t)ytab[y] * sw + xtab[x]];
}

// float bilinear up-resize of the depth plane (run_model_node.cpp:100-104); taps from the host.
__global__ __launch_bounds__(256) void resize_bilinear_f32_kernel(const float* src, int sw, const int* yi, const float* yf,
                                                                  const int* xi, const float* xf, int oh, int ow, float* dst) {
  // No FMA contraction here (the definition rounds every product and sum).  ROCm's __fmul_rn/__fadd_rn are plain
  // '*' and '+' compiled with contraction allowed inside their own bodies, so the arithmetic is spelled out with
  // operators under a lexically scoped contract(off).
#pragma clang fp contract(off)
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= ow) return;
  const int x0 = xi[2 * x], x1 = xi[2 * x + 1], y0 = yi[2 * y], y1 = yi[2 * y + 1];
  const float a0 = xf[2 * x], a1 = xf[2 * x + 1], b0 = yf[2 * y], b1 = yf[2 * y + 1];
  const float p00 = src[(size_t)y0 * sw + x0] * a0, p01 = src[(size_t)y0 * sw + x1] * a1;
  const float p10 = src[(size_t)y1 * sw + x0] * a0, p11 = src[(size_t)y1 * sw + x1] * a1;
  const float h0 = p00 + p01, h1 = p10 + p11;
  const float q0 = h0 * b0, q1 = h1 * b1;
  dst[(size_t)y * ow + x] = q0 + q1;
}

// ------------------------------------------------------------------------------ depth visualisation
// DepthVisualizationEngine::visualize (depth_visualization_engine.cpp:9-26): minMaxLoc -> convertTo(CV_8U, 255/(max-min),
// -min*255/(max-min)) -> applyColorMap(VIRIDIS).  Two launches over the frame-size fp32 depth plane.
// Order-preserving float -> unsigned key, so that min / max are integer atomics (exact, order-independent).
__device__ inline unsigned f32_order_key(float f) {
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline float f32_from_order_key(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// Range probe on a network's output: flags[blockIdx.x] = 1 if any value this workgroup scanned is inf / NaN, else 0.  The parity mode carries
// fp16 EXPONENT range (hi = fp16(x) overflows to inf above 65504); an overflow anywhere in the network reaches the logits as inf or NaN
// (inf - inf in the next convolution), so one pass over the 2.4 MB of logits (reads served by the L2 right behind the head's stores)
// catches it.  Every pass OVERWRITES all VP_PROBE_BLOCKS words (round 5): nothing is sticky, so no clear -- neither a memset node in the
// captured graph nor a host-side one -- stands between a bad frame and the good frame behind it; the host ORs the words it fetched.
__global__ __launch_bounds__(256) void finite_probe_kernel(const float* src, size_t n, unsigned* flags) {
  bool bad = false;
  const size_t n4 = n >> 2;
  const f32x4_t* s4 = reinterpret_cast<const f32x4_t*>(src);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const f32x4_t v = s4[i];
#pragma unroll
    for (int r = 0; r < 4; ++r) bad |= (__float_as_uint(v[r]) & 0x7F800000u) == 0x7F800000u;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) bad |= (__float_as_uint(src[(n4 << 2) + threadIdx.x]) & 0x7F800000u) == 0x7F800000u;
  __shared__ unsigned s_any;
  if (threadIdx.x == 0) s_any = 0u;
  __syncthreads();
  if (bad) s_any = 1u;   // every writer stores the same value
  __syncthreads();
  if (threadIdx.x == 0) flags[blockIdx.x] = s_any;
}

__global__ __launch_bounds__(256) void minmax_f32_kernel(const float* src, size_t n, unsigned* mm) {  // mm[0] = min key, mm[1] = max key
  __shared__ unsigned smin[4], smax[4];
  unsigned lo = 0xFFFFFFFFu, hi = 0u;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const unsigned k = f32_order_key(src[i]);
    lo = k < lo ? k : lo;
    hi = k > hi ? k : hi;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  if ((threadIdx.x & 63) == 0) {
    smin[threadIdx.x >> 6] = lo;
    smax[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < 4; ++q) {
      lo = smin[q] < lo ? smin[q] : lo;
      hi = smax[q] > hi ? smax[q] : hi;
    }
    atomicMin(mm, lo);
    atomicMax(mm + 1, hi);
  }
}

// u8 = saturate(cvRound(x * alpha + beta)) with alpha, beta formed in double and applied in float, as cv::Mat::convertTo does
// (fused multiply-add, the AVX2 / NEON build's v_fma; cvRound = round-half-even), then the 256 x BGR table.
__device__ __forceinline__ int depth_level(float x, float mn, float mx) {
  if (!(mx > mn)) return 0;
  const double range = (double)mx - (double)mn;
  const float a = (float)(255.0 / range), b = (float)(-(double)mn * 255.0 / range);
  const int r = __float2int_rn(__builtin_fmaf(x, a, b));
  return r < 0 ? 0 : (r > 255 ? 255 : r);
}
__global__ __launch_bounds__(256) void depth_colorize_kernel(const float* src, size_t n, const unsigned* mm, const uint8_t* lut, uint8_t* dst) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int v = depth_level(src[i], f32_from_order_key(mm[0]), f32_from_order_key(mm[1]));
  dst[3 * i] = lut[3 * v];
  dst[3 * i + 1] = lut[3 * v + 1];
  dst[3 * i + 2] = lut[3 * v + 2];
}

// ------------------------------------------------------------------------------------------ vp_canvas: overlays drawn in place
// kernels.hpp CanvasBlendParams: a work-item owns the aligned four-pixel block j of a canvas row, reads its three words, changes the pixels that are
// its to change and stores the three words again.  One work-item per block and launches in stream order: the pixels it merely carries are not raced for.
__device__ __forceinline__ void load_bgr4(const uint8_t* row, int j, unsigned px[4]) {
  const uint32_t* s = reinterpret_cast<const uint32_t*>(row + 12 * (size_t)j);
  const unsigned a = s[0], b = s[1], c = s[2];
  px[0] = a & 0xFFFFFFu;
  px[1] = (a >> 24) | ((b & 0xFFFFu) << 8);
  px[2] = (b >> 16) | ((c & 0xFFu) << 16);
  px[3] = c >> 8;
}
// the mask overlay of viz_blend_kernel on a region: same label, same LUT, same blend; the frame is the canvas itself and always BGR
__global__ __launch_bounds__(256) void canvas_blend_kernel(const CanvasBlendParams p) {
  const int jb0 = p.x0 >> 2, nb = ((p.x0 + p.w - 1) >> 2) - jb0 + 1;
  const int i = blockIdx.x * 256 + threadIdx.x, ry = blockIdx.y;
  if (i >= nb) return;
  const int j = jb0 + i;
  uint8_t* row = p.canvas + (size_t)(p.y0 + ry) * p.pitch;
  const uint8_t* mrow = p.mask + (size_t)p.ytab[ry] * p.mw;
  unsigned px[4];
  load_bgr4(row, j, px);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int rx = 4 * j + k - p.x0;
    if (rx < 0 || rx >= p.w) continue;   // the region's edge inside a block: carried, not drawn
    const uint8_t* c = p.lut + 3 * (int)mrow[p.xtab[rx]];
    px[k] = blend_half_even(c[0], px[k] & 255u) | (blend_half_even(c[1], (px[k] >> 8) & 255u) << 8) | (blend_half_even(c[2], px[k] >> 16) << 16);
  }
  store_bgr4(row, j, px);
}
// drawUntrackedDetection's box (autospeed_visualization_engine.cpp:126-140) without the text, kernels.hpp CanvasBoxParams
__device__ __forceinline__ unsigned fill_fifth(unsigned colour, unsigned d) { return (2u * colour + 8u * d + 5u) / 10u; }   // nearest to (colour + 4 d) / 5
__global__ __launch_bounds__(256) void canvas_boxes_kernel(const CanvasBoxParams p) {
  const int jb0 = p.ux0 >> 2, nb = (p.ux1 >> 2) - jb0 + 1;
  const int i = blockIdx.x * 256 + threadIdx.x, y = p.uy0 + (int)blockIdx.y;
  if (i >= nb) return;
  const int j = jb0 + i;
  uint8_t* row = p.canvas + (size_t)y * p.pitch;
  unsigned px[4];
  load_bgr4(row, j, px);
  for (int b = 0; b < p.n; ++b) {
    const CanvasBox q = p.box[b];
    if (y < q.y0 || y > q.y1) continue;
    const bool yedge = y == q.y0 || y == q.y1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = 4 * j + k;
      if (x < q.x0 || x > q.x1 || x < p.ux0 || x > p.ux1) continue;   // ux: inside the canvas
      if (yedge || x == q.x0 || x == q.x1)
        px[k] = q.bgr;
      else
        px[k] = fill_fifth(q.bgr & 255u, px[k] & 255u) | (fill_fifth((q.bgr >> 8) & 255u, (px[k] >> 8) & 255u) << 8) |
                (fill_fifth(q.bgr >> 16, px[k] >> 16) << 16);
    }
  }
  store_bgr4(row, j, px);
}
// depth_colorize_kernel into a region of the canvas (opaque)
__global__ __launch_bounds__(256) void canvas_depth_kernel(const float* src, const unsigned* mm, const uint8_t* lut, uint8_t* canvas, int pitch, int x0,
                                                           int y0, int w, int h) {
  const int jb0 = x0 >> 2, nb = ((x0 + w - 1) >> 2) - jb0 + 1;
  const int i = blockIdx.x * 256 + threadIdx.x, ry = blockIdx.y;
  if (i >= nb) return;
  const int j = jb0 + i;
  const float mn = f32_from_order_key(mm[0]), mx = f32_from_order_key(mm[1]);
  uint8_t* row = canvas + (size_t)(y0 + ry) * pitch;
  unsigned px[4];
  load_bgr4(row, j, px);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int rx = 4 * j + k - x0;
    if (rx < 0 || rx >= w) continue;
    const uint8_t* c = lut + 3 * depth_level(src[(size_t)ry * w + rx], mn, mx);
    px[k] = (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16);
  }
  store_bgr4(row, j, px);
}
// drawRawMasksInPlace's additive overlays (visualize.cpp:312-388) as one clamped sum per pixel, kernels.hpp CanvasAddPlanesParams
__device__ __forceinline__ unsigned add_sat8(unsigned d, unsigned s) { return min(255u, d + s); }
__global__ __launch_bounds__(256) void canvas_add_planes_kernel(const CanvasAddPlanesParams p) {
  const int jb0 = p.x0 >> 2, nb = ((p.x0 + p.w - 1) >> 2) - jb0 + 1;
  const int i = blockIdx.x * 256 + threadIdx.x, ry = blockIdx.y;
  if (i >= nb) return;
  const int j = jb0 + i;
  uint8_t* row = p.canvas + (size_t)(p.y0 + ry) * p.pitch;
  const float* mrow = p.planes + (size_t)p.ytab[ry] * p.mw;
  unsigned px[4];
  load_bgr4(row, j, px);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int rx = 4 * j + k - p.x0;
    if (rx < 0 || rx >= p.w) continue;   // the region's edge inside a block: carried, not drawn
    const float* m = mrow + p.xtab[rx];
    unsigned sb = 0u, sg = 0u, sr = 0u;
#pragma unroll
    for (int q = 0; q < kCanvasMaxPlanes; ++q) {
      if (q < p.n_planes && m[(size_t)q * p.plane_stride] > p.threshold) {   // NaN compares false
        sb += p.add[q] & 255u;
        sg += (p.add[q] >> 8) & 255u;
        sr += p.add[q] >> 16;
      }
    }
    px[k] = add_sat8(px[k] & 255u, sb) | (add_sat8((px[k] >> 8) & 255u, sg) << 8) | (add_sat8(px[k] >> 16, sr) << 16);
  }
  store_bgr4(row, j, px);
}
// filled discs of one colour, kernels.hpp CanvasPointParams; with p.rows the points are the valid rows of an AutoSteer engine's device logits
// (make_visualization, Models/visualizations/AutoSteer/video_visualization.py:19-44)
__global__ __launch_bounds__(256) void canvas_points_kernel(const CanvasPointParams p) {
  const int jb0 = p.ux0 >> 2, nb = (p.ux1 >> 2) - jb0 + 1;
  const int i = blockIdx.x * 256 + threadIdx.x, y = p.uy0 + (int)blockIdx.y;
  if (i >= nb) return;
  const int j = jb0 + i, r = p.radius;
  uint8_t* row = p.canvas + (size_t)y * p.pitch;
  unsigned px[4];
  load_bgr4(row, j, px);
  for (int b = 0; b < p.n; ++b) {
    int cx, cy;
    if (p.rows) {
      const float v = __fmul_rn(p.rows[b], 1024.0f);
      if (!(p.rows[p.n + b] >= 0.5f) || !(v > -1e8f && v < 1e8f)) continue;   // an invalid row; NaN or no pixel position
      cx = p.ox + (int)v;
      cy = p.oy + b * 511 / 63;
    } else {
      cx = p.pt[b].x;
      cy = p.pt[b].y;
    }
    const int dy = y - cy;
    if (dy < -r || dy > r) continue;
    const int lim = r * r - dy * dy;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = 4 * j + k, dx = x - cx;
      if (x < p.ux0 || x > p.ux1 || dx < -r || dx > r) continue;   // ux: inside the canvas
      if (dx * dx <= lim) px[k] = p.bgr;
    }
  }
  store_bgr4(row, j, px);
}
// preprocess_kernel's u8 value from one BGR8 picture into another, kernels.hpp CanvasResizeParams
__global__ __launch_bounds__(256) void canvas_resize_kernel(const CanvasResizeParams p) {
  const int j = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (j >= (p.out_w + 3) >> 2) return;
  const int4 yt = *reinterpret_cast<const int4*>(p.ytab + 4 * y);
  const uint8_t* r0 = p.src + (size_t)yt.x * p.src_pitch;
  const uint8_t* r1 = p.src + (size_t)yt.y * p.src_pitch;
  unsigned px[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = 4 * j + k;
    if (x >= p.out_w) break;
    const int4 xt = *reinterpret_cast<const int4*>(p.xtab + 4 * x);
    px[k] = (unsigned)bilinear_u8(r0, r1, xt, yt, 0) | ((unsigned)bilinear_u8(r0, r1, xt, yt, 1) << 8) | ((unsigned)bilinear_u8(r0, r1, xt, yt, 2) << 16);
  }
  store_bgr4(p.dst + (size_t)y * p.dst_pitch, j, px);
}
// Canvas -> a vp_frame format (kernels.hpp CanvasToFormatParams).  The forward form, the integer counterpart of the upload formula above, with the
// constants p.k of the canvas's colour standard (include/vp_hip.h states it as the DEFINITION; not pinned against OpenCV):
//   Y = sat8((yk . (R, G, B) + (off << 20) + 2^19) >> 20),  U = sat8((uk . (R, G, B) + (128 << 20) + 2^19) >> 20),  V likewise with vk
// In full range pure blue / pure red reach 256 before the clamp: there sat8 decides.
__device__ __forceinline__ unsigned luma_of(const BgrToYuv& k, unsigned px) {
  const int b = px & 255u, g = (px >> 8) & 255u, r = px >> 16;
  return sat8((k.yk[0] * r + k.yk[1] * g + k.yk[2] * b + (k.off << 20) + (1 << 19)) >> 20);
}
// U | V << 8, bits 16 .. 31 zero.  V is pinned in a register of its own: left to itself the backend packs the two shift-and-clamp steps into one
// v_ashr_pk_u8_i32 and then takes bits 16 .. 31 of that result for zero; on the MI355X they were not (the NV12 / I420 bytes of a block's second group came
// back OR-ed with them).
__device__ __forceinline__ unsigned chroma_of(const BgrToYuv& k, unsigned px) {
  const int b = px & 255u, g = (px >> 8) & 255u, r = px >> 16;
  unsigned v = sat8((k.vk[0] * r + k.vk[1] * g + k.vk[2] * b + (128 << 20) + (1 << 19)) >> 20);
  asm volatile("" : "+v"(v));
  return sat8((k.uk[0] * r + k.uk[1] * g + k.uk[2] * b + (128 << 20) + (1 << 19)) >> 20) | (v << 8);
}
// VP_CHROMA_MEAN: U | V << 8 of the n = 2 or 4 such (clamped) pairs of a group, (sum + n / 2) / n per component
__device__ __forceinline__ unsigned chroma_mean2(unsigned a, unsigned b) {
  const unsigned u = (a & 255u) + (b & 255u) + 1u, v = (a >> 8) + (b >> 8) + 1u;
  return (u >> 1) | ((v >> 1) << 8);
}
__device__ __forceinline__ unsigned chroma_mean4(unsigned a, unsigned b, unsigned c, unsigned d) {
  const unsigned u = (a & 255u) + (b & 255u) + (c & 255u) + (d & 255u) + 2u, v = (a >> 8) + (b >> 8) + (c >> 8) + (d >> 8) + 2u;
  return (u >> 2) | ((v >> 2) << 8);
}
__device__ __forceinline__ unsigned swap_rb(unsigned px) { return (px & 0x00FF00u) | (px >> 16) | ((px & 255u) << 16); }
__global__ __launch_bounds__(256) void canvas_to_format_kernel(const CanvasToFormatParams p) {
  const int bpr = (p.w + 3) >> 2;
  const bool f420 = p.format == 5 || p.format >= 16;       // NV12, I420 (YV12 arrives as I420), NV21
  const int rows = f420 ? p.h >> 1 : p.h;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)rows * bpr) return;
  const int r = (int)(t / bpr), j = (int)(t - (long long)r * bpr), x0 = 4 * j;
  const size_t pitch = (size_t)p.dst_pitch;
  unsigned px[4];
  if (f420) {   // rows 2r, 2r + 1; chroma of the top-left pixel of each 2x2 block, or the mean of the block's four
    unsigned px1[4], y0 = 0u, y1 = 0u, uv[2] = {0u, 0u};
    load_bgr4(p.src + (size_t)(2 * r) * p.src_pitch, j, px);
    load_bgr4(p.src + (size_t)(2 * r + 1) * p.src_pitch, j, px1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (x0 + k >= p.w) break;
      y0 |= luma_of(p.k, px[k]) << (8 * k);
      y1 |= luma_of(p.k, px1[k]) << (8 * k);
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      if (x0 + 2 * g >= p.w) break;                        // w is even: a group is whole or absent
      const unsigned c = chroma_of(p.k, px[2 * g]);
      uv[g] = p.chroma_mean ? chroma_mean4(c, chroma_of(p.k, px[2 * g + 1]), chroma_of(p.k, px1[2 * g]), chroma_of(p.k, px1[2 * g + 1])) : c;
    }
    *reinterpret_cast<uint32_t*>(p.p0 + (size_t)(2 * r) * pitch + 4 * (size_t)j) = y0;
    *reinterpret_cast<uint32_t*>(p.p0 + (size_t)(2 * r + 1) * pitch + 4 * (size_t)j) = y1;
    const size_t crow = (size_t)r * p.dst_pitch_c;
    if (p.format == 16) {   // I420: a plane each, this block's two samples as one 16-bit store
      *reinterpret_cast<uint16_t*>(p.p1 + crow + 2 * (size_t)j) = (uint16_t)((uv[0] & 255u) | ((uv[1] & 255u) << 8));
      *reinterpret_cast<uint16_t*>(p.p2 + crow + 2 * (size_t)j) = (uint16_t)((uv[0] >> 8) | ((uv[1] >> 8) << 8));
    } else {                // NV12: U V pairs; NV21: V U
      if (p.format == 18) {
        uv[0] = (uv[0] >> 8) | ((uv[0] & 255u) << 8);
        uv[1] = (uv[1] >> 8) | ((uv[1] & 255u) << 8);
      }
      *reinterpret_cast<uint32_t*>(p.p1 + crow + 4 * (size_t)j) = uv[0] | (uv[1] << 16);
    }
    return;
  }
  load_bgr4(p.src + (size_t)r * p.src_pitch, j, px);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (x0 + k >= p.w) px[k] = 0u;   // behind the row's end: zero bytes out, whatever the canvas carries there
  uint8_t* drow = p.p0 + (size_t)r * pitch;
  if (p.format >= 6) {   // YUY2: Y0 U Y1 V; UYVY: U Y0 V Y1 -- one word per pixel pair, chroma of the even pixel or the mean of the pair
    uint32_t* d = reinterpret_cast<uint32_t*>(drow + 8 * (size_t)j);
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      unsigned wd = 0u;
      if (x0 + 2 * g < p.w) {
        const unsigned ya = luma_of(p.k, px[2 * g]), yb = luma_of(p.k, px[2 * g + 1]);
        unsigned c = chroma_of(p.k, px[2 * g]);
        if (p.chroma_mean) c = chroma_mean2(c, chroma_of(p.k, px[2 * g + 1]));
        wd = p.format == 6 ? (ya | ((c & 255u) << 8) | (yb << 16) | ((c >> 8) << 24)) : ((c & 255u) | (ya << 8) | ((c >> 8) << 16) | (yb << 24));
      }
      d[g] = wd;
    }
  } else if (p.format == 4) {   // GRAY8 = Y
    unsigned wd = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (x0 + k < p.w) wd |= luma_of(p.k, px[k]) << (8 * k);
    *reinterpret_cast<uint32_t*>(drow + 4 * (size_t)j) = wd;
  } else if (p.format >= 2) {   // BGRA8 / RGBA8: alpha 255
    uint32_t* d = reinterpret_cast<uint32_t*>(drow + 16 * (size_t)j);
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = x0 + k < p.w ? ((p.format == 3 ? swap_rb(px[k]) : px[k]) | 0xFF000000u) : 0u;
  } else {                      // RGB8 (BGR8 is copied, not converted)
#pragma unroll
    for (int k = 0; k < 4; ++k) px[k] = swap_rb(px[k]);
    store_bgr4(drow, j, px);
  }
}

// ------------------------------------------------------------------------------------------ vp_canvas: the picture as a baseline JPEG
// kernels.hpp JpegBlocksParams / JpegEntropyParams; include/vp_hip.h states the stream.  One 8-point pass of the integer DCT:
// out[k] = (sum_n M[k][n] x[n] + round) >> shift with M[k][n] = rne(2^13 s_k cos((2n + 1) k pi / 16)); fully unrolled, M becomes immediates.
__device__ __forceinline__ void jpeg_dct8(const int x[8], int out[8], int round, int shift) {
  constexpr int M[8][8] = {{2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},      {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
                           {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784},  {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
                           {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896},  {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
                           {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567},  {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    int s = round;
#pragma unroll
    for (int n = 0; n < 8; ++n) s += M[k][n] * x[n];
    out[k] = s >> shift;
  }
}
// luma_of in a register of its own, for the reason chroma_of pins V: four of them are packed into one word below.  Unpinned, the backend merges a pair of
// shift-and-clamp steps into one v_ashr_pk_u8_i32 and ORs the other two samples into bits 16 .. 31 of its result, which it takes for zero; on the MI355X
// they are not.
__device__ __forceinline__ unsigned luma_pinned(const BgrToYuv& k, unsigned px) {
  unsigned v = luma_of(k, px);
  asm volatile("" : "+v"(v));
  return v;
}
__global__ __launch_bounds__(256) void jpeg_blocks_kernel(const JpegBlocksParams p) {
  constexpr int G = kJpegMcusPerGroup, BP = kJpegBlockPitch, NB = 6 * G;
  __shared__ int4 lds_a[NB * BP / 8];   // samples, then the row pass in place
  __shared__ int4 lds_b[NB * BP / 8];   // quantised coefficients in zigzag order
  __shared__ int lds_q[128];
  int16_t* sa = reinterpret_cast<int16_t*>(lds_a);
  int16_t* sb = reinterpret_cast<int16_t*>(lds_b);
  const int tid = threadIdx.x, mcu0 = (int)blockIdx.x * G;
  if (tid < 128) lds_q[tid] = p.q[tid >> 6][tid & 63];
  {   // load: MCU m, row pair r, four-pixel block j
    const int m = tid >> 5, r = (tid >> 2) & 7, j = tid & 3, mcu = mcu0 + m;
    if (mcu < p.n_mcus) {
      const int my = mcu / p.mcus_x, mx = mcu - my * p.mcus_x;
      const int gp = 8 * my + r, hp = p.h >> 1, gpc = min(gp, hp - 1);
      const int jb = 4 * mx + j, jbc = min(jb, (p.w - 1) >> 2);
      unsigned px[4], px1[4];
      load_bgr4(p.src + (size_t)(2 * gpc) * p.src_pitch, jbc, px);
      load_bgr4(p.src + (size_t)(2 * gpc + 1) * p.src_pitch, jbc, px1);
      unsigned ya = 0u, yb = 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        ya |= luma_pinned(p.k, px[k]) << (8 * k);
        yb |= luma_pinned(p.k, px1[k]) << (8 * k);
      }
      if (gp >= hp) ya = yb;   // both rows lie below the picture: row h - 1 again
      const unsigned c0 = chroma_mean4(chroma_of(p.k, px[0]), chroma_of(p.k, px[1]), chroma_of(p.k, px1[0]), chroma_of(p.k, px1[1]));
      const unsigned c1 = chroma_mean4(chroma_of(p.k, px[2]), chroma_of(p.k, px[3]), chroma_of(p.k, px1[2]), chroma_of(p.k, px1[3]));
      int16_t* yblk = sa + (6 * m + (r >= 4 ? 2 : 0) + (j >> 1)) * BP + ((2 * r) & 7) * 8 + (j & 1) * 4;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int sx = min(4 * jb + k, p.w - 1) - 4 * jbc;   // 0 .. 3: the pixel of the loaded block this sample repeats
        yblk[k] = (int16_t)((int)((ya >> (8 * sx)) & 255u) - 128);
        yblk[8 + k] = (int16_t)((int)((yb >> (8 * sx)) & 255u) - 128);
        if (!(k & 1)) {
          const unsigned c = (sx >> 1) ? c1 : c0;
          sa[(6 * m + 4) * BP + r * 8 + 2 * j + (k >> 1)] = (int16_t)((int)(c & 255u) - 128);
          sa[(6 * m + 5) * BP + r * 8 + 2 * j + (k >> 1)] = (int16_t)((int)(c >> 8) - 128);
        }
      }
    }
  }
  __syncthreads();
  for (int u = tid; u < 8 * NB; u += 256) {   // rows: T[y][k] = (sum_n M[k][n] x[y][n] + 2^9) >> 10, in place
    const int b = u >> 3, y = u & 7;
    if (mcu0 + b / 6 >= p.n_mcus) continue;
    int4* row = lds_a + (b * BP + y * 8) / 8;
    const int4 v = *row;
    const int x[8] = {(int16_t)v.x, v.x >> 16, (int16_t)v.y, v.y >> 16, (int16_t)v.z, v.z >> 16, (int16_t)v.w, v.w >> 16};
    int t[8];
    jpeg_dct8(x, t, 1 << 9, 10);
    int4 o;
    o.x = (t[0] & 0xFFFF) | (int)((unsigned)t[1] << 16);
    o.y = (t[2] & 0xFFFF) | (int)((unsigned)t[3] << 16);
    o.z = (t[4] & 0xFFFF) | (int)((unsigned)t[5] << 16);
    o.w = (t[6] & 0xFFFF) | (int)((unsigned)t[7] << 16);
    *row = o;
  }
  __syncthreads();
  for (int u = tid; u < 8 * NB; u += 256) {   // columns: F[l][k] = (sum_m M[l][m] T[m][k] + 2^15) >> 16, quantised into its zigzag place
    constexpr uint8_t kPlace[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                    10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
    const int b = u >> 3, k = u & 7;
    if (mcu0 + b / 6 >= p.n_mcus) continue;
    const int* q = lds_q + (b % 6 >= 4 ? 64 : 0);
    int x[8], f[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) x[m] = sa[b * BP + m * 8 + k];
    jpeg_dct8(x, f, 1 << 15, 16);
#pragma unroll
    for (int l = 0; l < 8; ++l) {
      const int Q = q[l * 8 + k], a = (abs(f[l]) + (Q >> 1)) / Q;
      int c = f[l] < 0 ? -a : a;
      if (l | k) c = min(max(c, -1023), 1023);
      sb[b * BP + kPlace[l * 8 + k]] = (int16_t)c;
    }
  }
  __syncthreads();
  int4* dst = reinterpret_cast<int4*>(p.coef) + (size_t)mcu0 * 48;
  for (int u = tid; u < 8 * NB; u += 256)
    if (mcu0 + (u >> 3) / 6 < p.n_mcus) dst[u] = lds_b[(u >> 3) * (BP / 8) + (u & 7)];
}
// One restart interval, coded serially (T.81 F.1.2).  The sink counts, or stores at dst: every byte that leaves the accumulator, a 0x00 behind each 0xFF.
template <bool WRITE>
struct JpegSink {
  uint8_t* dst;
  unsigned n;
  unsigned long long acc;
  int nb;
  __device__ __forceinline__ void put(unsigned bits, int len) {   // len <= 26 on top of fewer than 8 pending bits
    acc = (acc << len) | bits;
    nb += len;
    while (nb >= 8) {
      const unsigned b = (unsigned)(acc >> (nb - 8)) & 255u;
      nb -= 8;
      if (WRITE) dst[n] = (uint8_t)b;
      ++n;
      if (b == 255u) {
        if (WRITE) dst[n] = 0;
        ++n;
      }
    }
  }
  __device__ __forceinline__ void symbol(unsigned entry, int v, int size) {   // a Huffman entry (code | length << 16), then the low `size` bits of v (v - 1 when negative)
    const unsigned extra = (unsigned)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
    put(((entry & 0xFFFFu) << size) | extra, (int)(entry >> 16) + size);
  }
};
__device__ __forceinline__ int jpeg_size_of(int v) {
  const unsigned a = (unsigned)abs(v);
  return a ? 32 - __builtin_clz(a) : 0;
}
// `huff` is the workgroup's LDS copy of the entries.  The eight 16-byte words of the NEXT block are loaded before the current block is coded, so that a
// work-item waits for memory once per block at the most, not once per word.
template <bool WRITE>
__device__ unsigned jpeg_code_interval(const int4* coef, int n_mcus, const uint32_t* huff, uint8_t* dst) {
  JpegSink<WRITE> s{dst, 0u, 0ull, 0};
  int pred_y = 0, pred_cb = 0, pred_cr = 0;
  const int n_blocks = 6 * n_mcus;
  int4 nxt[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) nxt[i] = coef[i];
  for (int t = 0, b = 0; t < n_blocks; ++t, b = b == 5 ? 0 : b + 1) {
    int4 w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = nxt[i];
    const int4* ahead = coef + (size_t)min(t + 1, n_blocks - 1) * 8;   // the last block once more: never past the interval
#pragma unroll
    for (int i = 0; i < 8; ++i) nxt[i] = ahead[i];
    const int comp = b < 4 ? 0 : b - 3;
    const uint32_t* dc = huff + (comp ? 16 : 0);
    const uint32_t* ac = huff + 32 + (comp ? 256 : 0);
    int run = 0;
#pragma unroll
    for (int wi = 0; wi < 8; ++wi) {
      const int4 v = w[wi];
      const int c[8] = {(int16_t)v.x, v.x >> 16, (int16_t)v.y, v.y >> 16, (int16_t)v.z, v.z >> 16, (int16_t)v.w, v.w >> 16};
      if (wi == 0) {
        const int d = c[0] - (comp == 0 ? pred_y : (comp == 1 ? pred_cb : pred_cr)), size = jpeg_size_of(d);
        if (comp == 0) pred_y = c[0];
        if (comp == 1) pred_cb = c[0];
        if (comp == 2) pred_cr = c[0];
        s.symbol(dc[size], d, size);
      }
      if (((wi == 0 ? v.x & (int)0xFFFF0000u : v.x) | v.y | v.z | v.w) == 0) {
        run += wi == 0 ? 7 : 8;
        continue;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (wi == 0 && e == 0) continue;
        if (c[e] == 0) {
          ++run;
          continue;
        }
        while (run > 15) {
          s.put(ac[0xF0] & 0xFFFFu, (int)(ac[0xF0] >> 16));
          run -= 16;
        }
        const int size = jpeg_size_of(c[e]);
        s.symbol(ac[(run << 4) | size], c[e], size);
        run = 0;
      }
    }
    if (run > 0) s.put(ac[0] & 0xFFFFu, (int)(ac[0] >> 16));
  }
  if (s.nb > 0) s.put((1u << (8 - s.nb)) - 1u, 8 - s.nb);
  return s.n;
}
template <bool WRITE>
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const JpegEntropyParams p) {
  __shared__ uint32_t lds_huff[kJpegHuffWords];
  for (int k = threadIdx.x; k < kJpegHuffWords; k += 64) lds_huff[k] = p.huff[k];
  __syncthreads();
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (i >= p.n_intervals) return;
  const int first = i * p.restart_mcus, n = min(p.restart_mcus, p.n_mcus - first);
  const int4* coef = reinterpret_cast<const int4*>(p.coef) + (size_t)first * 48;
  const bool marker = i + 1 < p.n_intervals;
  if (WRITE) {
    uint8_t* dst = p.out + p.len[i];
    const unsigned bytes = jpeg_code_interval<true>(coef, n, lds_huff, dst);
    if (marker) {
      dst[bytes] = 0xFF;
      dst[bytes + 1] = (uint8_t)(0xD0 + (i & 7));
    }
  } else {
    p.len[i] = jpeg_code_interval<false>(coef, n, lds_huff, nullptr) + (marker ? 2u : 0u);
  }
}
// len[0, n) -> its exclusive prefix sum, in place; *total = the sum.  One workgroup: a chunk per work-item, the 256 chunk sums scanned through LDS.
__global__ __launch_bounds__(256) void jpeg_scan_kernel(uint32_t* len, int n, uint32_t* total) {
  __shared__ unsigned part[2][256];
  const int tid = threadIdx.x, chunk = (n + 255) / 256, lo = min(n, tid * chunk), hi = min(n, lo + chunk);
  unsigned sum = 0u;
  for (int i = lo; i < hi; ++i) sum += len[i];
  part[0][tid] = sum;
  __syncthreads();
  int cur = 0;
  for (int d = 1; d < 256; d <<= 1) {
    part[cur ^ 1][tid] = part[cur][tid] + (tid >= d ? part[cur][tid - d] : 0u);
    cur ^= 1;
    __syncthreads();
  }
  unsigned at = part[cur][tid] - sum;
  for (int i = lo; i < hi; ++i) {
    const unsigned l = len[i];
    len[i] = at;
    at += l;
  }
  if (tid == 255) *total = part[cur][255];
}

// ----------------------------------------------------------------------------------- layout conversions
// fp32 NCHW (host-visible test/debug format) <-> NHWC activation.
__global__ __launch_bounds__(256) void nchw_to_act_kernel(const float* src, int Creal, ActView a) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int HW = a.H * a.W;
  if (t >= (long long)HW * a.C) return;
  const int c = (int)(t % a.C), pix = (int)(t / a.C);
  const float v = c < Creal ? src[(size_t)c * HW + pix] : 0.0f;
  const half_t h = (half_t)v;
  a.hi[t] = h;
  if (a.lo) a.lo[t] = (half_t)(v - (float)h);
}
__global__ __launch_bounds__(256) void act_to_nchw_kernel(ActView a, int Creal, float* dst, float mul) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int HW = a.H * a.W;
  if (t >= (long long)HW * Creal) return;
  const int pix = (int)(t % HW), c = (int)(t / HW);
  const size_t off = (size_t)pix * a.C + c;
  float v = (float)a.hi[off];
  if (a.lo) v += (float)a.lo[off];
  dst[t] = v * mul;   // mul = 1 (exact) unless the tensor is stored scaled (VP_ACT_SCALE)
}

// VP_ACT_SCALE calibration: max |hi + lo| and the count of non-finite elements of one tensor.  A thread reads one 16-byte octet per plane; octets that
// straddle the real-channel count are masked per element (the padding of an alias slice belongs to its neighbour).  |x| >= 0 as fp32 orders like its bit
// pattern, so the maximum is an INTEGER max (wave shuffle, then one atomicMax per wave) and the count an integer add: order-independent, no float atomics.
__global__ __launch_bounds__(256) void act_absmax_kernel(const half_t* hi, const half_t* lo, int c, long long npix, int c_pitch, unsigned* result) {
  const int CG = (c + 7) >> 3;
  unsigned best = 0u, bad = 0u;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < npix * CG; t += (long long)gridDim.x * 256) {
    const int cg = (int)(t % CG);
    const size_t off = (size_t)(t / CG) * c_pitch + cg * 8;
    const h8_t h = *reinterpret_cast<const h8_t*>(hi + off);
    h8_t l = {};
    if (lo) l = *reinterpret_cast<const h8_t*>(lo + off);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (cg * 8 + i >= c) continue;
      const unsigned u = __float_as_uint((float)h[i] + (float)l[i]) & 0x7FFFFFFFu;
      if (u >= 0x7F800000u) ++bad;
      else best = u > best ? u : best;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned b2 = __shfl_xor(best, o);
    best = b2 > best ? b2 : best;
    bad += __shfl_xor(bad, o);
  }
  if ((threadIdx.x & 63) == 0) {
    if (best) atomicMax(result, best);
    if (bad) atomicAdd(result + 1, bad);
  }
}

// Range survey (vp_range_survey): counts the stored values x = (float)hi + (float)lo of one tensor per binary exponent.  result[k], k < VP_HIST_BINS:
// elements with floor(log2 |x|) == VP_HIST_EXP_MIN + k; result[VP_HIST_BINS]: exact zeros (+0 and -0); result[VP_HIST_BINS + 1]: real elements visited.
// Non-finite elements are counted in neither a bin nor the zeros (act_absmax_kernel counts them); pad channels are left out by that kernel's rule, and
// the loads are its loads: one 16-byte octet per plane and thread.  The exponent is read off the fp32 bits: a non-zero sum of two fp16 values is a
// multiple of 2^-24, hence a normal fp32 number.  A finite sum of 2^16 or more -- no (hi, lo) pair an engine stores reaches it, only arbitrary planes
// handed to the operator entry can -- is counted in the top bin, so that bins + zeros + non-finite always add up to the element count.
// In a real tensor almost all values fall into three or four adjacent bins, so a shared histogram would serialise a wave on one address.  Here every
// LANE owns a sub-histogram in LDS, laid out [wave][counter pair][lane]: the word of (pair, lane) lies in bank `lane` whatever the bin, so one
// ds_add_u32 per element is conflict-free for every value distribution, and nobody else touches a lane's words (no barrier until the end).  Two
// 16-bit counters share a word (the add is 1 or 1 << 16): 21 words per lane, 21.5 KB per workgroup instead of 42, which is what lets seven
// workgroups share a CU and keep act_absmax_kernel's number of loads in flight.  A 16-bit counter holds a lane's share as long as the lane visits
// fewer than 2^16 elements; the launcher sizes the grid for that (kHistOctetsPerThread).  At the end a wave sums its 64 sub-histograms by shuffles,
// the block's four waves meet in LDS, and one thread per counter adds the block's sum to global memory with an ordinary vector atomic on the 64-bit
// word (at most 42 per block).  All sums are integer: the result does not depend on the order, two runs give equal words.
constexpr long long kHistOctetsPerThread = 8191;   // 8 elements each: 65528 < 2^16
__global__ __launch_bounds__(256) void act_exp_hist_kernel(const half_t* hi, const half_t* lo, int c, long long npix, int c_pitch, unsigned long long* result) {
  constexpr int NB = VP_HIST_BINS + 1;   // the bins, then the zeros
  constexpr int NW = (NB + 1) / 2;       // words per lane: counter b is the (b & 1) half of word b >> 1
  __shared__ unsigned hist[4][NW][64];
  __shared__ unsigned long long wsum[4][NB + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned(*mine)[64] = hist[wave];
#pragma unroll
  for (int b = 0; b < NW; ++b) mine[b][lane] = 0u;
  const int CG = (c + 7) >> 3;
  unsigned seen = 0u;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < npix * CG; t += (long long)gridDim.x * 256) {
    const int cg = (int)(t % CG);
    const size_t off = (size_t)(t / CG) * c_pitch + cg * 8;
    const h8_t h = *reinterpret_cast<const h8_t*>(hi + off);
    h8_t l = {};
    if (lo) l = *reinterpret_cast<const h8_t*>(lo + off);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (cg * 8 + i >= c) continue;
      ++seen;
      const unsigned u = __float_as_uint((float)h[i] + (float)l[i]) & 0x7FFFFFFFu;
      if (u >= 0x7F800000u) continue;
      int b = (int)(u >> 23) - (127 + VP_HIST_EXP_MIN);
      b = u == 0u ? VP_HIST_BINS : (b > VP_HIST_BINS - 1 ? VP_HIST_BINS - 1 : (b < 0 ? 0 : b));
      atomicAdd(&mine[b >> 1][lane], 1u << ((b & 1) << 4));   // the lane's own word: one ds_add_u32, no return value
    }
  }
#pragma unroll 1
  for (int b = 0; b <= NB; ++b) {
    unsigned long long v = b < NB ? ((mine[b >> 1][lane] >> ((b & 1) << 4)) & 0xFFFFu) : seen;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) wsum[wave][b] = v;
  }
  __syncthreads();
  if (threadIdx.x <= NB) {
    const unsigned long long v = wsum[0][threadIdx.x] + wsum[1][threadIdx.x] + wsum[2][threadIdx.x] + wsum[3][threadIdx.x];
    if (v) atomicAdd(result + threadIdx.x, v);
  }
}

// ---------------------------------------------------------------------------------------------- launchers
hipError_t launch_preprocess(const PreprocessParams& p, hipStream_t st) {
  VP_LAUNCH(preprocess_kernel, dim3(nblk(p.out_w), p.out_h), dim3(256), 0, st, p);
}
hipError_t launch_frame_to_bgr8(const FrameToBgrParams& q, hipStream_t st) {
  FrameToBgrParams p = q;
  const bool pairs = p.format >= 5, f420 = frame_format_420(p.format);   // 4:2:x: whole chroma groups only
  if (!p.p0 || !p.dst || frame_format_index(p.format) < 0 || p.h < 2 || p.w < 2 || (pairs && (p.w & 1)) || (f420 && (!p.p1 || (p.h & 1))) ||
      (frame_format_planar(p.format) && !p.p2) || p.dst_pitch < frame_bgr_pitch(p.w) || (p.dst_pitch & 3) || (reinterpret_cast<uintptr_t>(p.dst) & 3))
    return hipErrorInvalidValue;
  if (p.format == 17) {   // YV12 = I420 with the chroma planes exchanged
    std::swap(p.p1, p.p2);
    std::swap(p.s1, p.s2);
    p.format = 16;
  }
  const long long n = (long long)(f420 ? p.h / 2 : p.h) * ((p.w + 3) / 4);
  VP_LAUNCH(frame_to_bgr8_kernel, dim3(nblk(n)), dim3(256), 0, st, p);
}
hipError_t launch_frame_deep_to_bgr8(const FrameDeepParams& p, hipStream_t st) {
  const bool p010 = p.format == 21;
  const auto odd = [](const void* a, int s) { return ((reinterpret_cast<uintptr_t>(a) | (uintptr_t)s) & 1) != 0; };
  if (!frame_format_deep(p.format) || !p.p0 || !p.dst || p.h < 2 || p.w < 2 || p.h > 16384 || p.w > 16384 || p.s0 < 2 * p.w || odd(p.p0, p.s0) ||
      (p010 && (!p.p1 || ((p.h | p.w) & 1) || p.s1 < 2 * p.w || odd(p.p1, p.s1))) || p.dst_pitch < frame_bgr_pitch(p.w) || (p.dst_pitch & 3) ||
      (reinterpret_cast<uintptr_t>(p.dst) & 3))
    return hipErrorInvalidValue;
  const long long n = (long long)(p010 ? p.h / 2 : p.h) * ((p.w + 3) / 4);
  VP_LAUNCH(frame_deep_to_bgr8_kernel, dim3(nblk(n)), dim3(256), 0, st, p);
}
hipError_t launch_frame_raw_to_bgr8(const FrameRawParams& p, hipStream_t st) {
  const int px_bytes = p.wide ? 2 : 1;
  bool ok = p.src && p.dst && p.h >= 2 && p.w >= 2 && p.h <= 16384 && p.w <= 16384 && !((p.h | p.w) & 1) && p.stride >= px_bytes * p.w &&
            (p.wide ? p.bits == 10 || p.bits == 12 || p.bits == 14 || p.bits == 16 : p.bits == 8) &&
            (!p.wide || !((reinterpret_cast<uintptr_t>(p.src) | (uintptr_t)p.stride) & 1)) && p.shift >= 0 && p.shift <= 8 && p.black >= 0 &&
            p.black < (1 << p.bits) && (p.wide | p.green00 | p.red_row0 | p.ccm_on | 1) == 1 && p.dst_pitch >= frame_bgr_pitch(p.w) && !(p.dst_pitch & 3) &&
            !(reinterpret_cast<uintptr_t>(p.dst) & 3);
  for (int g : p.gains) ok = ok && g >= 0 && g <= 16383;         // 65535 * 16383 + 128 < 2^31
  for (int c : p.ccm) ok = ok && (!p.ccm_on || (c >= -8191 && c <= 8191));   // 3 * 8191 * 65535 + 512 < 2^31
  if (!ok) return hipErrorInvalidValue;
  VP_LAUNCH(frame_raw_to_bgr8_kernel, dim3(nblk((long long)(p.h / 2) * ((p.w + 3) / 4))), dim3(256), 0, st, p);
}
hipError_t launch_frame_remap(const FrameRemapParams& p, hipStream_t st) {
  if (!p.src || !p.map || !p.dst || p.src_h < 1 || p.src_w < 1 || p.src_h > 32768 || p.src_w > 32768 || p.src_pitch < 3 * p.src_w || p.out_h < 1 || p.out_w < 1 ||
      p.out_h > 16384 || p.out_w > 16384 || p.map_pitch < frame_remap_map_pitch(p.out_w) || (p.map_pitch & 3) || (reinterpret_cast<uintptr_t>(p.map) & 15) ||
      (p.border != 0 && p.border != 1) || p.dst_pitch < frame_bgr_pitch(p.out_w) || (p.dst_pitch & 3) || (reinterpret_cast<uintptr_t>(p.dst) & 3))
    return hipErrorInvalidValue;
  VP_LAUNCH(frame_remap_kernel, dim3(nblk((p.out_w + 3) / 4), p.out_h), dim3(256), 0, st, p);
}
hipError_t launch_pil_resample(const PilResampleParams& p, hipStream_t st) {
  hipLaunchKernelGGL(pil_resample_h_kernel, dim3(nblk(p.out_w), p.in_h), dim3(256), 0, st, p);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  VP_LAUNCH(pil_resample_v_kernel, dim3(nblk(p.out_w), p.out_h), dim3(256), 0, st, p);
}
bool ctx_exp_conv1_ok(const CtxExpConv1Params& q) {
  const FcParams& p = q.fc;
  const bool g_ok = q.glanes >= 1 && q.glanes <= 64 && (q.glanes & (q.glanes - 1)) == 0;
  return (q.tile == 2 || q.tile == 8 || q.tile == 16) && g_ok && p.K >= 4 && (p.K & 3) == 0 && p.N == q.cv.H * q.cv.W && (p.w != nullptr) != (p.w8 != nullptr) && p.b && q.cv.w && q.cv.b &&
         (q.cv.out.C & 7) == 0 && p.act_rows == 0 && (p.partial != nullptr || p.x != nullptr) && (size_t)(((p.K + 3) & ~3) + (q.tile + 2) * (q.tile + 2)) * 4 <= 48 * 1024;
}
hipError_t launch_ctx_exp_conv1(const CtxExpConv1Params& q, hipStream_t st) {
  if (!ctx_exp_conv1_ok(q)) return hipErrorInvalidValue;
  const int T = q.tile;
  const unsigned grid = (unsigned)(((q.cv.H + T - 1) / T) * ((q.cv.W + T - 1) / T));
  const size_t lds = (size_t)(((q.fc.K + 3) & ~3) + (T + 2) * (T + 2)) * sizeof(float);
  if (T == 16) {
    VP_LAUNCH(ctx_exp_conv1_kernel<16>, dim3(grid), dim3(256), lds, st, q);
  }
  if (T == 2) {
    VP_LAUNCH(ctx_exp_conv1_kernel<2>, dim3(grid), dim3(256), lds, st, q);
  }
  VP_LAUNCH(ctx_exp_conv1_kernel<8>, dim3(grid), dim3(256), lds, st, q);
}
hipError_t launch_ctx_conv1(const CtxConv1Params& p, hipStream_t st) {
  VP_LAUNCH(ctx_conv1_kernel, dim3(nblk((long long)p.H * p.W * (p.out.C >> 3))), dim3(256), 0, st, p);
}
bool fusion_octets_ok(const FusionParams& p) {
  int units = 0, creal = 0;
  for (int l = 0; l < 5; ++l) {
    if ((p.creal[l] & 7) || p.shift[l] < 0 || p.shift[l] > 6) return false;
    const int n2 = 1 << (2 * p.shift[l]);
    units += (p.creal[l] >> 3) * (n2 < 16 ? n2 : 16);
    creal += p.creal[l];
  }
  return units <= 512 && creal == p.Creal_out && (p.Creal_out & 7) == 0 && (p.out.C & 7) == 0;
}
hipError_t launch_fusion(const FusionParams& p, hipStream_t st) {
  if (p.octets) {
    if (!fusion_octets_ok(p)) return hipErrorInvalidValue;
    VP_LAUNCH(fusion_octet_kernel, dim3(p.out.H * p.out.W), dim3(256), 0, st, p);
  }
  VP_LAUNCH(fusion_kernel, dim3(nblk((long long)p.out.H * p.out.W * p.out.C)), dim3(256), 0, st, p);
}
hipError_t launch_decode_mask(const float* logits, int C, int HW, int mode, uint8_t* out, hipStream_t st) {
  VP_LAUNCH(decode_mask_kernel, dim3(nblk(HW)), dim3(256), 0, st, logits, C, HW, mode, out);
}
hipError_t launch_resize_nearest(const uint8_t* src, int sw, const int* ytab, const int* xtab, int oh, int ow, uint8_t* dst,
                                 hipStream_t st) {
  VP_LAUNCH(resize_nearest_kernel, dim3(nblk(ow), oh), dim3(256), 0, st, src, sw, ytab, xtab, oh, ow, dst);
}
hipError_t launch_viz_blend(const uint8_t* mask, int mw, const int* ytab, const int* xtab, const uint8_t* frame, int stride, int oh, int ow,
                            const uint8_t* lut, int frame_is_rgb, uint8_t* dst, hipStream_t st) {
  VP_LAUNCH(viz_blend_kernel, dim3(nblk(ow), oh), dim3(256), 0, st, mask, mw, ytab, xtab, frame, stride, oh, ow, lut, frame_is_rgb, dst);
}
hipError_t launch_minmax_f32(const float* src, size_t n, unsigned* mm, hipStream_t st) {
  const unsigned blocks = (unsigned)((n + 255) / 256);
  VP_LAUNCH(minmax_f32_kernel, dim3(blocks < 1024u ? (blocks ? blocks : 1u) : 1024u), dim3(256), 0, st, src, n, mm);
}
hipError_t launch_finite_probe(const float* src, size_t n, unsigned* flags, hipStream_t st) {
  VP_LAUNCH(finite_probe_kernel, dim3(VP_PROBE_BLOCKS), dim3(256), 0, st, src, n, flags);  // always the full grid: every word is rewritten
}
hipError_t launch_depth_colorize(const float* src, size_t n, const unsigned* mm, const uint8_t* lut, uint8_t* dst, hipStream_t st) {
  VP_LAUNCH(depth_colorize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, n, mm, lut, dst);
}
hipError_t launch_resize_bilinear_f32(const float* src, int sw, const int* yi, const float* yf, const int* xi, const float* xf,
                                      int oh, int ow, float* dst, hipStream_t st) {
  VP_LAUNCH(resize_bilinear_f32_kernel, dim3(nblk(ow), oh), dim3(256), 0, st, src, sw, yi, yf, xi, xf, oh, ow, dst);
}
// a region drawn in place: inside the canvas, the canvas with the pitch and alignment the three-word blocks need
static bool canvas_region_ok(const uint8_t* canvas, int pitch, int canvas_h, int canvas_w, int x0, int y0, int w, int h) {
  return canvas && canvas_h >= 1 && canvas_w >= 1 && pitch >= frame_bgr_pitch(canvas_w) && !(pitch & 3) && !(reinterpret_cast<uintptr_t>(canvas) & 3) && x0 >= 0 &&
         y0 >= 0 && w >= 1 && h >= 1 && (long long)x0 + w <= canvas_w && (long long)y0 + h <= canvas_h;
}
hipError_t launch_canvas_blend(const CanvasBlendParams& p, int canvas_h, int canvas_w, hipStream_t st) {
  if (!p.mask || !p.ytab || !p.xtab || !p.lut || p.mw < 1 || !canvas_region_ok(p.canvas, p.pitch, canvas_h, canvas_w, p.x0, p.y0, p.w, p.h)) return hipErrorInvalidValue;
  const int nb = ((p.x0 + p.w - 1) >> 2) - (p.x0 >> 2) + 1;
  VP_LAUNCH(canvas_blend_kernel, dim3(nblk(nb), p.h), dim3(256), 0, st, p);
}
hipError_t launch_canvas_boxes(const CanvasBoxParams& p, int canvas_h, int canvas_w, hipStream_t st) {
  if (p.n < 1 || p.n > kCanvasBoxChunk || p.ux1 < p.ux0 || p.uy1 < p.uy0 ||
      !canvas_region_ok(p.canvas, p.pitch, canvas_h, canvas_w, p.ux0, p.uy0, p.ux1 - p.ux0 + 1, p.uy1 - p.uy0 + 1))
    return hipErrorInvalidValue;
  const int nb = (p.ux1 >> 2) - (p.ux0 >> 2) + 1;
  VP_LAUNCH(canvas_boxes_kernel, dim3(nblk(nb), p.uy1 - p.uy0 + 1), dim3(256), 0, st, p);
}
hipError_t launch_canvas_depth(const float* src, const unsigned* mm, const uint8_t* lut, uint8_t* canvas, int pitch, int x0, int y0, int w, int h,
                               int canvas_h, int canvas_w, hipStream_t st) {
  if (!src || !mm || !lut || !canvas_region_ok(canvas, pitch, canvas_h, canvas_w, x0, y0, w, h)) return hipErrorInvalidValue;
  const int nb = ((x0 + w - 1) >> 2) - (x0 >> 2) + 1;
  VP_LAUNCH(canvas_depth_kernel, dim3(nblk(nb), h), dim3(256), 0, st, src, mm, lut, canvas, pitch, x0, y0, w, h);
}
hipError_t launch_canvas_add_planes(const CanvasAddPlanesParams& p, int canvas_h, int canvas_w, hipStream_t st) {
  if (!p.planes || !p.ytab || !p.xtab || p.n_planes < 1 || p.n_planes > kCanvasMaxPlanes || p.mw < 1 || p.plane_stride < p.mw || !(p.threshold == p.threshold) ||
      (reinterpret_cast<uintptr_t>(p.planes) & 3) || !canvas_region_ok(p.canvas, p.pitch, canvas_h, canvas_w, p.x0, p.y0, p.w, p.h))
    return hipErrorInvalidValue;
  const int nb = ((p.x0 + p.w - 1) >> 2) - (p.x0 >> 2) + 1;
  VP_LAUNCH(canvas_add_planes_kernel, dim3(nblk(nb), p.h), dim3(256), 0, st, p);
}
hipError_t launch_canvas_points(const CanvasPointParams& p, int canvas_h, int canvas_w, hipStream_t st) {
  if (p.n < 1 || p.n > kCanvasPointChunk || p.radius < 0 || p.radius > kCanvasMaxRadius || p.ux1 < p.ux0 || p.uy1 < p.uy0 || (reinterpret_cast<uintptr_t>(p.rows) & 3) ||
      !canvas_region_ok(p.canvas, p.pitch, canvas_h, canvas_w, p.ux0, p.uy0, p.ux1 - p.ux0 + 1, p.uy1 - p.uy0 + 1))
    return hipErrorInvalidValue;
  const int nb = (p.ux1 >> 2) - (p.ux0 >> 2) + 1;
  VP_LAUNCH(canvas_points_kernel, dim3(nblk(nb), p.uy1 - p.uy0 + 1), dim3(256), 0, st, p);
}
hipError_t launch_canvas_resize(const CanvasResizeParams& p, hipStream_t st) {
  if (!p.src || !p.dst || !p.xtab || !p.ytab || p.src_h < 1 || p.src_w < 1 || p.src_pitch < 3 * p.src_w || p.out_h < 1 || p.out_w < 1 || p.out_h > 16384 || p.out_w > 16384 ||
      p.dst_pitch < frame_bgr_pitch(p.out_w) || (p.dst_pitch & 3) || (reinterpret_cast<uintptr_t>(p.dst) & 3) ||
      ((reinterpret_cast<uintptr_t>(p.xtab) | reinterpret_cast<uintptr_t>(p.ytab)) & 15))
    return hipErrorInvalidValue;
  VP_LAUNCH(canvas_resize_kernel, dim3(nblk((p.out_w + 3) / 4), p.out_h), dim3(256), 0, st, p);
}
hipError_t launch_canvas_to_format(const CanvasToFormatParams& q, hipStream_t st) {
  CanvasToFormatParams p = q;
  const bool pairs = p.format >= 5, f420 = frame_format_420(p.format);
  if (!p.src || !p.p0 || p.format < 1 || frame_format_index(p.format) < 0 || p.h < 1 || p.w < 1 || (pairs && (p.w & 1)) || (f420 && (!p.p1 || (p.h & 1))) ||
      (frame_format_planar(p.format) && !p.p2) || p.src_pitch < frame_bgr_pitch(p.w) || (p.src_pitch & 3) || p.dst_pitch != canvas_plane_pitch(p.format, p.w) ||
      (f420 && p.dst_pitch_c != canvas_plane_pitch(p.format, p.w, 1)) ||
      ((reinterpret_cast<uintptr_t>(p.src) | reinterpret_cast<uintptr_t>(p.p0) | reinterpret_cast<uintptr_t>(p.p1) | reinterpret_cast<uintptr_t>(p.p2)) & 3))
    return hipErrorInvalidValue;
  if (p.format == 17) {   // YV12 = I420 with the chroma planes exchanged
    std::swap(p.p1, p.p2);
    p.format = 16;
  }
  const long long n = (long long)(f420 ? p.h / 2 : p.h) * ((p.w + 3) / 4);
  VP_LAUNCH(canvas_to_format_kernel, dim3(nblk(n)), dim3(256), 0, st, p);
}
hipError_t launch_jpeg_blocks(const JpegBlocksParams& p, hipStream_t st) {
  if (!p.src || !p.coef || p.h < 2 || p.w < 2 || p.h > 16384 || p.w > 16384 || ((p.h | p.w) & 1) || p.src_pitch < frame_bgr_pitch(p.w) || (p.src_pitch & 3) ||
      p.mcus_x != (p.w + 15) / 16 || p.n_mcus != p.mcus_x * ((p.h + 15) / 16) || ((reinterpret_cast<uintptr_t>(p.src) & 3) | (reinterpret_cast<uintptr_t>(p.coef) & 15)))
    return hipErrorInvalidValue;
  for (int i = 0; i < 128; ++i)
    if (p.q[i >> 6][i & 63] == 0) return hipErrorInvalidValue;
  VP_LAUNCH(jpeg_blocks_kernel, dim3((unsigned)((p.n_mcus + kJpegMcusPerGroup - 1) / kJpegMcusPerGroup)), dim3(256), 0, st, p);
}
hipError_t launch_jpeg_entropy(const JpegEntropyParams& p, bool write, hipStream_t st) {
  if (!p.coef || !p.huff || !p.len || (write && !p.out) || p.n_mcus < 1 || p.restart_mcus < 1 || p.restart_mcus > 65535 ||
      p.n_intervals != (p.n_mcus + p.restart_mcus - 1) / p.restart_mcus || (reinterpret_cast<uintptr_t>(p.coef) & 15))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((p.n_intervals + 63) / 64));
  if (write) VP_LAUNCH(jpeg_entropy_kernel<true>, grid, dim3(64), 0, st, p);
  VP_LAUNCH(jpeg_entropy_kernel<false>, grid, dim3(64), 0, st, p);
}
hipError_t launch_jpeg_scan(uint32_t* len, int n, uint32_t* total, hipStream_t st) {
  if (!len || !total || n < 1) return hipErrorInvalidValue;
  VP_LAUNCH(jpeg_scan_kernel, dim3(1), dim3(256), 0, st, len, n, total);
}
hipError_t launch_nchw_to_act(const float* src, int Creal, const ActView& a, hipStream_t st) {
  VP_LAUNCH(nchw_to_act_kernel, dim3(nblk((long long)a.H * a.W * a.C)), dim3(256), 0, st, src, Creal, a);
}
hipError_t launch_act_absmax(const half_t* hi, const half_t* lo, int c, int h, int w, int c_pitch, unsigned* result, hipStream_t st) {
  if (!hi || !result || c < 1 || h < 1 || w < 1 || c_pitch < ((c + 7) & ~7) || (c_pitch & 7) || ((reinterpret_cast<uintptr_t>(hi) | reinterpret_cast<uintptr_t>(lo)) & 15))
    return hipErrorInvalidValue;
  const long long n = (long long)h * w * ((c + 7) >> 3);
  const unsigned blocks = n > 1024ll * 256 ? 1024u : (unsigned)((n + 255) / 256);
  VP_LAUNCH(act_absmax_kernel, dim3(blocks), dim3(256), 0, st, hi, lo, c, (long long)h * w, c_pitch, result);
}
hipError_t launch_act_exp_hist(const half_t* hi, const half_t* lo, int c, int h, int w, int c_pitch, unsigned long long* result, hipStream_t st) {
  if (!hi || !result || c < 1 || h < 1 || w < 1 || c_pitch < ((c + 7) & ~7) || (c_pitch & 7) || ((reinterpret_cast<uintptr_t>(hi) | reinterpret_cast<uintptr_t>(lo)) & 15))
    return hipErrorInvalidValue;
  const long long n = (long long)h * w * ((c + 7) >> 3);   // the grid of launch_act_absmax: the same octets per thread, the same bytes read ...
  long long blocks = n > 1024ll * 256 ? 1024 : (n + 255) / 256;
  const long long need = (n + 256 * kHistOctetsPerThread - 1) / (256 * kHistOctetsPerThread);   // ... unless a lane's 16-bit counters would not hold its share (beyond 2^34 elements)
  if (need > blocks) blocks = need;
  if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
  VP_LAUNCH(act_exp_hist_kernel, dim3((unsigned)blocks), dim3(256), 0, st, hi, lo, c, (long long)h * w, c_pitch, result);
}
hipError_t launch_act_to_nchw(const ActView& a, int Creal, float* dst, hipStream_t st, float mul) {
  VP_LAUNCH(act_to_nchw_kernel, dim3(nblk((long long)a.H * a.W * Creal)), dim3(256), 0, st, a, Creal, dst, mul);
}

// ------------------------------------------------------------------------------------------ vp_metric
// The validation scores of Models/training/scene_seg_trainer.py:206-244, domain_seg_trainer.py:236-252 and scene_3d_trainer.py:94-109, 159-210,
// restated (kernels.hpp: the rules every kernel here follows).
// calc_IoU_val's cascade: the first maximum for finite logits; a NaN fails every branch (3: no class)
__device__ __forceinline__ int metric_class3(float a, float b, float c) { return (a >= b && a >= c) ? 0 : ((b >= a && b >= c) ? 1 : ((c >= a && c >= b) ? 2 : 3)); }
__device__ __forceinline__ bool metric_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }
// one pixel: pred 0 .. 2 or 3 (none), truth a mask of planes; cnt = I[3] P[3] G[3]
__device__ __forceinline__ void metric_count(int pred, unsigned truth, unsigned* cnt) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const unsigned p = pred == k, g = (truth >> k) & 1u;
    cnt[k] += p & g;
    cnt[3 + k] += p;
    cnt[6 + k] += g;
  }
}
__device__ __forceinline__ unsigned metric_truth(unsigned v, int c, int gt_form) {
  if (gt_form) return v & (c == 3 ? 7u : 1u);
  return c == 3 ? (v < 3u ? 1u << v : 0u) : (v ? 1u : 0u);
}
__global__ __launch_bounds__(256) void metric_seg_count_kernel(const MetricSegParams p) {
  __shared__ unsigned wave_cnt[4][10];
  unsigned cnt[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) cnt[k] = 0;
  const unsigned n = p.n;
  const float* l0 = p.logits;
  const float* r0 = p.ref;
  // four pixels per step where every plane starts on a 16-byte boundary
  const bool vec = !(n & 3u) && !((reinterpret_cast<uintptr_t>(l0) | reinterpret_cast<uintptr_t>(r0)) & 15) && !(reinterpret_cast<uintptr_t>(p.gt) & 3);
  const unsigned nq = vec ? n >> 2 : 0u;
  for (unsigned q = blockIdx.x * 256 + threadIdx.x; q < nq; q += gridDim.x * 256) {
    int4 l[3], r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      l[k].x = l[k].y = l[k].z = l[k].w = 0;
      r[k] = l[k];
      if (k < p.c) l[k] = *reinterpret_cast<const int4*>(l0 + (size_t)k * n + 4 * (size_t)q);
      if (r0 && k < p.c) r[k] = *reinterpret_cast<const int4*>(r0 + (size_t)k * n + 4 * (size_t)q);
    }
    const unsigned gt4 = p.gt ? *reinterpret_cast<const unsigned*>(p.gt + 4 * (size_t)q) : 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float a[3], b[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        a[k] = __uint_as_float((unsigned)(j == 0 ? l[k].x : j == 1 ? l[k].y : j == 2 ? l[k].z : l[k].w));
        b[k] = __uint_as_float((unsigned)(j == 0 ? r[k].x : j == 1 ? r[k].y : j == 2 ? r[k].z : r[k].w));
      }
      int pred;
      unsigned truth;
      if (p.c == 3) {
        pred = metric_class3(a[0], a[1], a[2]);
        cnt[9] += pred == 3;
        const int rc = r0 ? metric_class3(b[0], b[1], b[2]) : 3;
        truth = r0 ? (rc < 3 ? 1u << rc : 0u) : metric_truth((gt4 >> (8 * j)) & 255u, 3, p.gt_form);
      } else {
        pred = a[0] > 0.0f ? 0 : 3;
        cnt[9] += a[0] != a[0];
        truth = r0 ? (b[0] > 0.0f ? 1u : 0u) : metric_truth((gt4 >> (8 * j)) & 255u, 1, p.gt_form);
      }
      metric_count(pred, truth, cnt);
    }
  }
  for (unsigned i = 4 * nq + blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    int pred;
    unsigned truth;
    if (p.c == 3) {
      pred = metric_class3(l0[i], l0[(size_t)n + i], l0[2 * (size_t)n + i]);
      cnt[9] += pred == 3;
      const int rc = r0 ? metric_class3(r0[i], r0[(size_t)n + i], r0[2 * (size_t)n + i]) : 3;
      truth = r0 ? (rc < 3 ? 1u << rc : 0u) : metric_truth(p.gt[i], 3, p.gt_form);
    } else {
      pred = l0[i] > 0.0f ? 0 : 3;
      cnt[9] += l0[i] != l0[i];
      truth = r0 ? (r0[i] > 0.0f ? 1u : 0u) : metric_truth(p.gt[i], 1, p.gt_form);
    }
    metric_count(pred, truth, cnt);
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt[k] += __shfl_xor(cnt[k], o);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 10; ++k) wave_cnt[threadIdx.x >> 6][k] = cnt[k];
  }
  __syncthreads();
  if (threadIdx.x < 10) {   // one integer atomic per workgroup per counter: the sum does not depend on the order
    const unsigned v = wave_cnt[0][threadIdx.x] + wave_cnt[1][threadIdx.x] + wave_cnt[2][threadIdx.x] + wave_cnt[3][threadIdx.x];
    if (v) atomicAdd(&p.rec->I[0] + threadIdx.x, v);
  }
  if (blockIdx.x == 0 && threadIdx.x == 10) {
    p.rec->kind = p.kind;
    p.rec->n = n;
  }
}

// one value per work-item of a 256-thread workgroup combined in a fixed tree (the same bits on every run); every work-item gets the result
template <class T, class Op>
__device__ __forceinline__ T metric_block_reduce(T v, T* lds, Op op) {
  lds[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) lds[threadIdx.x] = op(lds[threadIdx.x], lds[threadIdx.x + o]);
    __syncthreads();
  }
  const T r = lds[0];
  __syncthreads();
  return r;
}
struct MetricStat {   // one plane's sum, extremes and non-finite count
  double sum;
  float mn, mx;
  unsigned bad;
};
struct MetricStatJoin {
  __device__ __forceinline__ MetricStat operator()(const MetricStat& a, const MetricStat& b) const {
    return MetricStat{a.sum + b.sum, b.mn < a.mn ? b.mn : a.mn, b.mx > a.mx ? b.mx : a.mx, a.bad + b.bad};
  }
};
struct MetricSumJoin {
  __device__ __forceinline__ double operator()(double a, double b) const { return a + b; }
};
// 1. min, max, sum and non-finite count of both planes: one partial per workgroup
__global__ __launch_bounds__(256) void metric_depth_stats_kernel(const MetricDepthParams p) {
  __shared__ MetricStat lds[256];
  const unsigned n = (unsigned)p.h * (unsigned)p.w;
  MetricStatPartial out;
  for (int j = 0; j < 2; ++j) {
    const float* src = j ? p.gt : p.pred;
    MetricStat s{0.0, INFINITY, -INFINITY, 0u};
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
      const float v = src[i];
      if (metric_finite(v)) {
        s.sum += (double)v;
        s.mn = v < s.mn ? v : s.mn;
        s.mx = v > s.mx ? v : s.mx;
      } else {
        ++s.bad;
      }
    }
    s = metric_block_reduce(s, lds, MetricStatJoin());
    out.sum[j] = s.sum;
    out.mn[j] = s.mn;
    out.mx[j] = s.mx;
    out.bad[j] = s.bad;
  }
  if (threadIdx.x == 0) p.stat[blockIdx.x] = out;
}
// the fold of the stats partials (nb <= 256, partial b through work-item b, the fixed tree): ssi(t) = (t - mn) / den with den = max - mean, all fp32
// (get_ssi_nom_tensor); bad: non-finite inputs.  Called by the whole workgroup.
struct MetricNorm {
  float mn[2], den[2];
  unsigned bad;
};
__device__ __forceinline__ MetricNorm metric_fold_stats(const MetricStatPartial* stat, unsigned nb, unsigned n, MetricStat* lds) {
  MetricNorm r;
  r.bad = 0;
  for (int j = 0; j < 2; ++j) {
    MetricStat s{0.0, INFINITY, -INFINITY, 0u};
    if (threadIdx.x < nb) s = MetricStat{stat[threadIdx.x].sum[j], stat[threadIdx.x].mn[j], stat[threadIdx.x].mx[j], stat[threadIdx.x].bad[j]};
    s = metric_block_reduce(s, lds, MetricStatJoin());
    r.bad += s.bad;
    r.mn[j] = s.mn;
    r.den[j] = __fsub_rn(s.mx, (float)(s.sum / (double)n));
  }
  return r;
}
// 2. D = ssi(pred) - ssi(gt) and the bits of |D|
__global__ __launch_bounds__(256) void metric_depth_diff_kernel(const MetricDepthParams p, unsigned nb_stat) {
  __shared__ MetricStat lds[256];
  const unsigned n = (unsigned)p.h * (unsigned)p.w;
  const MetricNorm nm = metric_fold_stats(p.stat, nb_stat, n, lds);
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float a = __fdiv_rn(__fsub_rn(p.pred[i], nm.mn[0]), nm.den[0]);
    const float b = __fdiv_rn(__fsub_rn(p.gt[i], nm.mn[1]), nm.den[1]);
    const float d = __fsub_rn(a, b);
    p.d[i] = d;
    p.a_bits[i] = __float_as_uint(d) & 0x7FFFFFFFu;
  }
}
// 3. radix select on u32 keys for two ranks at once, most significant byte first.  Launch `pass` (0 .. 3) first folds the histograms launch pass - 1
// left (every workgroup repeats that fold; workgroup 0 stores the state for the launch after it), then counts byte `pass` of the keys that carry the
// chosen prefix into an LDS histogram and stores it as its partial; launch 4 (one workgroup) folds the last histograms and stores the two keys.
// A work-item counts runs of equal digits before it touches LDS: the keys of |D| share their exponent byte almost everywhere.
// scratch: state [5][4] (prefix0, prefix1, rest0, rest1 ahead of pass s), then partial [4 passes][nb][2][256].
constexpr int kMetricSelState = 32;   // words in front of the partials
__global__ __launch_bounds__(256) void metric_select_pass_kernel(const unsigned* bits, unsigned n, unsigned k0, unsigned k1, int pass, unsigned nb, unsigned* scratch,
                                                                 unsigned* out) {
  __shared__ unsigned hist[2][256];
  __shared__ unsigned scan[2][256];
  __shared__ unsigned st[4];
  const unsigned t = threadIdx.x;
  unsigned* state = scratch;
  unsigned* partial = scratch + kMetricSelState;
  if (t == 0) {
    st[0] = pass >= 2 ? state[4 * (pass - 1)] : 0u;
    st[1] = pass >= 2 ? state[4 * (pass - 1) + 1] : 0u;
    st[2] = pass >= 2 ? state[4 * (pass - 1) + 2] : k0;
    st[3] = pass >= 2 ? state[4 * (pass - 1) + 3] : k1;
  }
  __syncthreads();
  if (pass >= 1) {   // the fold of pass - 1: column sums in workgroup order, an inclusive scan, the bin that holds the rank
    const bool both = st[0] != st[1];
    const unsigned* src = partial + (size_t)(pass - 1) * nb * 512;
    unsigned h[2] = {0u, 0u};
    for (unsigned b = 0; b < nb; ++b) {
      h[0] += src[(size_t)b * 512 + t];
      if (both) h[1] += src[(size_t)b * 512 + 256 + t];
    }
    if (!both) h[1] = h[0];
    scan[0][t] = h[0];
    scan[1][t] = h[1];
    __syncthreads();
    for (unsigned o = 1; o < 256; o <<= 1) {
      const unsigned v0 = t >= o ? scan[0][t - o] : 0u, v1 = t >= o ? scan[1][t - o] : 0u;
      __syncthreads();
      scan[0][t] += v0;
      scan[1][t] += v1;
      __syncthreads();
    }
    const unsigned r0 = st[2], r1 = st[3], p0 = st[0], p1 = st[1];
    const unsigned e0 = scan[0][t] - h[0], e1 = scan[1][t] - h[1];
    __syncthreads();
    if (h[0] && e0 <= r0 && r0 < e0 + h[0]) {   // exactly one work-item: the rank lies below the total
      st[0] = (p0 << 8) | t;
      st[2] = r0 - e0;
    }
    if (h[1] && e1 <= r1 && r1 < e1 + h[1]) {
      st[1] = (p1 << 8) | t;
      st[3] = r1 - e1;
    }
    __syncthreads();
    if (blockIdx.x == 0 && t < 4 && pass < 4) state[4 * pass + t] = st[t];
  }
  if (pass == 4) {
    if (t < 2) out[t] = st[t];
    return;
  }
  const int shift = 24 - 8 * pass;
  hist[0][t] = 0;
  hist[1][t] = 0;
  __syncthreads();
  const unsigned p0 = st[0], p1 = st[1];
  const bool both = p0 != p1;   // one histogram serves both ranks while their prefixes agree
  unsigned last = 0, run = 0;
  for (unsigned i = blockIdx.x * 256 + t; i < n; i += gridDim.x * 256) {
    const unsigned v = bits[i];
    const unsigned hi = pass ? v >> (shift + 8) : 0u;
    const unsigned key = (hi == p0 ? 256u : 0u) | ((both && hi == p1) ? 512u : 0u) | ((v >> shift) & 255u);
    if (key == last) {
      ++run;
      continue;
    }
    if (run && (last & 256u)) atomicAdd(&hist[0][last & 255u], run);
    if (run && (last & 512u)) atomicAdd(&hist[1][last & 255u], run);
    last = key;
    run = 1;
  }
  if (run && (last & 256u)) atomicAdd(&hist[0][last & 255u], run);
  if (run && (last & 512u)) atomicAdd(&hist[1][last & 255u], run);
  __syncthreads();
  unsigned* dst = partial + ((size_t)pass * nb + blockIdx.x) * 512;
  dst[t] = hist[0][t];
  dst[256 + t] = hist[1][t];
}
// torch.quantile's interpolation (lerp): a + w (b - a) below w = 0.5, b - (b - a)(1 - w) from there on; fp32
__device__ __forceinline__ float metric_quantile(float a, float b, float w) {
  const float d = __fsub_rn(b, a);
  return w < 0.5f ? __fadd_rn(a, __fmul_rn(w, d)) : __fsub_rn(b, __fmul_rn(d, __fsub_rn(1.0f, w)));
}
// 4a. the kept set {A < q}: count and sum (double) per workgroup
__global__ __launch_bounds__(256) void metric_depth_kept_kernel(const MetricDepthParams p, float w) {
  __shared__ double lds[256];
  const unsigned n = (unsigned)p.h * (unsigned)p.w;
  const float q = metric_quantile(__uint_as_float(p.sel[0]), __uint_as_float(p.sel[1]), w);
  double s = 0.0, c = 0.0;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float a = __uint_as_float(p.a_bits[i]);
    if (a < q) {
      s += (double)a;
      c += 1.0;
    }
  }
  s = metric_block_reduce(s, lds, MetricSumJoin());
  c = metric_block_reduce(c, lds, MetricSumJoin());   // counts below 2^24: exact
  if (threadIdx.x == 0) p.kept[blockIdx.x] = MetricKeptPartial{s, (unsigned long long)c};
}
// 4b. one scale: sum of |Gx(src)| + |Gy(src)| (the 3x3 filters of scene_3d_trainer.py:96-106, zero padding 1) per workgroup, and the 2x2 mean pool of src
// (stride 2, a trailing odd row / column dropped) into dst (null at the last scale)
__device__ __forceinline__ float metric_at(const float* s, int h, int w, int y, int x) { return (y >= 0 && y < h && x >= 0 && x < w) ? s[(size_t)y * w + x] : 0.0f; }
__global__ __launch_bounds__(256) void metric_depth_edge_kernel(const float* src, int h, int w, float* dst, double* partial) {
  __shared__ double lds[256];
  const unsigned n = (unsigned)h * (unsigned)w;
  double s = 0.0;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int y = (int)(i / (unsigned)w), x = (int)(i % (unsigned)w);
    const float a00 = metric_at(src, h, w, y - 1, x - 1), a01 = metric_at(src, h, w, y - 1, x), a02 = metric_at(src, h, w, y - 1, x + 1);
    const float a10 = metric_at(src, h, w, y, x - 1), a12 = metric_at(src, h, w, y, x + 1);
    const float a20 = metric_at(src, h, w, y + 1, x - 1), a21 = metric_at(src, h, w, y + 1, x), a22 = metric_at(src, h, w, y + 1, x + 1);
    const float gx = __fadd_rn(__fmul_rn(0.125f, __fadd_rn(__fsub_rn(a00, a02), __fsub_rn(a20, a22))), __fmul_rn(0.25f, __fsub_rn(a10, a12)));
    const float gy = __fadd_rn(__fmul_rn(0.125f, __fadd_rn(__fsub_rn(a00, a20), __fsub_rn(a02, a22))), __fmul_rn(0.25f, __fsub_rn(a01, a21)));
    s += (double)__fadd_rn(fabsf(gx), fabsf(gy));
  }
  s = metric_block_reduce(s, lds, MetricSumJoin());
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
  if (!dst) return;
  const int h2 = h >> 1, w2 = w >> 1;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < (unsigned)h2 * (unsigned)w2; i += gridDim.x * 256) {
    const float* r0 = src + (size_t)(2 * (i / (unsigned)w2)) * w + 2 * (i % (unsigned)w2);
    dst[i] = __fmul_rn(0.25f, __fadd_rn(__fadd_rn(r0[0], r0[1]), __fadd_rn(r0[w], r0[w + 1])));
  }
}
// 5. the record: the partials folded in the fixed tree, means as one fp32 division each (sums below 2^24 ulps of their terms are exact in the double)
struct MetricFinishParams {
  unsigned nb_stat, nb_kept, nb_edge[4], n_edge[4];
  float w;
};
__global__ __launch_bounds__(256) void metric_depth_finish_kernel(const MetricDepthParams p, const MetricFinishParams f) {
  __shared__ MetricStat lds_stat[256];
  __shared__ double lds[256];
  const unsigned n = (unsigned)p.h * (unsigned)p.w, t = threadIdx.x;
  const MetricNorm nm = metric_fold_stats(p.stat, f.nb_stat, n, lds_stat);
  const double ks = metric_block_reduce(t < f.nb_kept ? p.kept[t].sum : 0.0, lds, MetricSumJoin());
  const double kc = metric_block_reduce(t < f.nb_kept ? (double)p.kept[t].count : 0.0, lds, MetricSumJoin());
  float mel = 0.0f;
  for (int s = 0; s < 4; ++s) {
    const double es = metric_block_reduce(t < f.nb_edge[s] ? p.edge[s * kMetricBlocks + t] : 0.0, lds, MetricSumJoin());
    mel = __fadd_rn(mel, __fdiv_rn((float)es, (float)f.n_edge[s]));
  }
  if (t != 0) return;
  MetricRecord r;
  r.kind = p.kind;
  for (int k = 0; k < 3; ++k) r.I[k] = r.P[k] = r.G[k] = 0;
  r.nonfinite = nm.bad;
  r.n = n;
  const float a = __uint_as_float(p.sel[0]), b = __uint_as_float(p.sel[1]);
  const float nan = __uint_as_float(0x7FC00000u);
  const bool bad = nm.bad != 0;
  r.kept = bad ? 0u : (unsigned)kc;
  r.q_lo = bad ? nan : a;
  r.q_hi = bad ? nan : b;
  r.q = bad ? nan : metric_quantile(a, b, f.w);
  r.mae = bad ? nan : __fdiv_rn((float)ks, (float)kc);   // an empty kept set: 0 / 0, the reference's empty mean
  r.mel = bad ? nan : __fmul_rn(mel, 0.25f);
  *p.rec = r;
}

hipError_t launch_metric_seg_count(const MetricSegParams& p, hipStream_t st) {
  if (!p.logits || !p.rec || (p.c != 1 && p.c != 3) || p.n < 1 || p.n > kMetricMaxN || (!p.gt && !p.ref) || (p.gt && p.ref) || (p.gt_form != 0 && p.gt_form != 1) ||
      ((reinterpret_cast<uintptr_t>(p.logits) | reinterpret_cast<uintptr_t>(p.ref)) & 3))
    return hipErrorInvalidValue;
  const unsigned blocks = nblk(((long long)p.n + 3) / 4);
  VP_LAUNCH(metric_seg_count_kernel, dim3(blocks < (unsigned)kMetricBlocks ? blocks : (unsigned)kMetricBlocks), dim3(256), 0, st, p);
}
static unsigned metric_select_blocks(unsigned n) {
  const unsigned b = (n + 4095) / 4096;   // sixteen keys per work-item, then more
  return b < (unsigned)kMetricBlocks ? b : (unsigned)kMetricBlocks;
}
size_t metric_select_scratch_bytes(unsigned n) { return sizeof(unsigned) * (kMetricSelState + (size_t)4 * metric_select_blocks(n) * 512); }
hipError_t launch_metric_select(const unsigned* bits, unsigned n, unsigned k0, unsigned k1, unsigned* scratch, unsigned* out, hipStream_t st) {
  if (!bits || !out || !scratch || n < 1 || n > kMetricMaxN || k0 >= n || k1 >= n) return hipErrorInvalidValue;
  const unsigned nb = metric_select_blocks(n);
  for (int pass = 0; pass < 4; ++pass) hipLaunchKernelGGL(metric_select_pass_kernel, dim3(nb), dim3(256), 0, st, bits, n, k0, k1, pass, nb, scratch, out);
  VP_LAUNCH(metric_select_pass_kernel, dim3(1), dim3(256), 0, st, bits, n, k0, k1, 4, nb, scratch, out);
}
size_t metric_pooled_elems(int h, int w) {
  size_t t = 0;
  for (int s = 0; s < 3; ++s) {
    h >>= 1;
    w >>= 1;
    t += (size_t)h * w;
  }
  return t;
}
static unsigned metric_blocks(size_t n) {
  const size_t b = (n + 255) / 256;
  return (unsigned)(b < (size_t)kMetricBlocks ? (b ? b : 1) : (size_t)kMetricBlocks);
}
hipError_t launch_metric_depth(const MetricDepthParams& p, hipStream_t st) {
  if (!p.pred || !p.gt || !p.d || !p.a_bits || !p.pooled || !p.stat || !p.kept || !p.edge || !p.sel || !p.sel_scratch || !p.rec || p.h < 8 || p.w < 8 ||
      (long long)p.h * p.w > (long long)kMetricMaxN)
    return hipErrorInvalidValue;
  const unsigned n = (unsigned)p.h * (unsigned)p.w, nb = metric_blocks(n);
  unsigned lo, hi;
  MetricFinishParams f{};
  metric_quantile_rank(n, &lo, &hi, &f.w);
  f.nb_stat = f.nb_kept = nb;
  hipLaunchKernelGGL(metric_depth_stats_kernel, dim3(nb), dim3(256), 0, st, p);
  hipLaunchKernelGGL(metric_depth_diff_kernel, dim3(nb), dim3(256), 0, st, p, nb);
  const hipError_t e = launch_metric_select(p.a_bits, n, lo, hi, p.sel_scratch, p.sel, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(metric_depth_kept_kernel, dim3(nb), dim3(256), 0, st, p, f.w);
  const float* src = p.d;
  float* dst = p.pooled;
  int h = p.h, w = p.w;
  for (int s = 0; s < 4; ++s) {
    f.n_edge[s] = (unsigned)h * (unsigned)w;
    f.nb_edge[s] = metric_blocks(f.n_edge[s]);
    hipLaunchKernelGGL(metric_depth_edge_kernel, dim3(f.nb_edge[s]), dim3(256), 0, st, src, h, w, s < 3 ? dst : (float*)nullptr, p.edge + s * kMetricBlocks);
    src = dst;
    h >>= 1;
    w >>= 1;
    dst += (size_t)h * w;
  }
  VP_LAUNCH(metric_depth_finish_kernel, dim3(1), dim3(256), 0, st, p, f);
}

// ------------------------------------------------------------------------------------------ vp_metric, lane part
// ego_lanes_trainer.py:280-356 and auto_steer_trainer.py:203-222, restated (kernels.hpp: the two shapes of the lanes chain, the rows' summation order).
constexpr int kLanesParts = 7;   // per plane: the BCE sum, five edge sums, the non-finite count
__device__ __forceinline__ double* metric_lanes_part(const MetricLanesParams& p, int c, int k) { return p.part + (size_t)(c * kLanesParts + k) * kMetricBlocks; }
// the ground truth of pixel (y, x) of plane c; *bad counts a non-finite value of the fp32 form
__device__ __forceinline__ float metric_lanes_gt(const MetricLanesParams& p, int c, int y, int x, unsigned* bad) {
  const size_t n = (size_t)p.h * p.w, i = (size_t)y * p.w + x;
  if (p.gt_form == kLanesGtPlanes) {
    const float v = static_cast<const float*>(p.gt)[c * n + i];
    *bad += !metric_finite(v);
    return v;
  }
  if (p.gt_form == kLanesGtRef) return static_cast<const float*>(p.gt)[c * n + i] > 0.0f ? 1.0f : 0.0f;
  unsigned v;
  if (p.gt_form == kLanesGtBits) {
    v = static_cast<const uint8_t*>(p.gt)[i];
  } else {   // the two 2x2 maximum pools of binary planes: the OR over the 4x4 block, four bytes per row (the launcher checks the alignment)
    const unsigned* q = reinterpret_cast<const unsigned*>(static_cast<const uint8_t*>(p.gt) + 16 * (size_t)y * p.w + 4 * (size_t)x);
    v = q[0] | q[p.w] | q[2 * (size_t)p.w] | q[3 * (size_t)p.w];
    v |= v >> 16;
    v |= v >> 8;
  }
  return (float)((v >> c) & 1u);
}
// one 2x2 cell of plane c: per pixel the BCEWithLogits term (1 - g) x + max(-x, 0) + log1p(exp(-|x|)) and D0 = R - g with R = relu(x); the mean of
// E = T - g over a whole cell into p1, T = Threshold(0, 1)(R): R where R > 0, 1 elsewhere.  A trailing odd row or column has cells of two pixels or one.
__device__ __forceinline__ void metric_lanes_cell(const MetricLanesParams& p, int c, int cy, int cx, float* d0, float* p1, double* bce, unsigned* bad) {
  const int h = p.h, w = p.w;
  const float* x0 = p.logits + (size_t)c * h * w;
  float e[2][2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int y = 2 * cy + j, x = 2 * cx + k;
      e[j][k] = 0.0f;
      if (y < h && x < w) {
        const float v = x0[(size_t)y * w + x];
        const float g = metric_lanes_gt(p, c, y, x, bad);
        *bad += !metric_finite(v);
        *bce += (double)__fadd_rn(__fmul_rn(__fsub_rn(1.0f, g), v), __fadd_rn(fmaxf(-v, 0.0f), log1pf(expf(-fabsf(v)))));
        const float r = v > 0.0f ? v : 0.0f;
        d0[(size_t)y * w + x] = __fsub_rn(r, g);
        e[j][k] = __fsub_rn(r > 0.0f ? r : 1.0f, g);
      }
    }
  }
  if (2 * cy + 1 < h && 2 * cx + 1 < w) p1[(size_t)cy * (w >> 1) + cx] = __fmul_rn(0.25f, __fadd_rn(__fadd_rn(e[0][0], e[0][1]), __fadd_rn(e[1][0], e[1][1])));
}
// the pixels first, first + step, ... of one scale: the sum of |Gx(src)| + |Gy(src)| (metric_depth_edge_kernel's filters and expression) and, with dst, the
// 2x2 mean pool of src
__device__ __forceinline__ double metric_lanes_edge_part(const float* src, int h, int w, float* dst, unsigned first, unsigned step) {
  const unsigned n = (unsigned)h * (unsigned)w;
  double s = 0.0;
  for (unsigned i = first; i < n; i += step) {
    const int y = (int)(i / (unsigned)w), x = (int)(i % (unsigned)w);
    const float a00 = metric_at(src, h, w, y - 1, x - 1), a01 = metric_at(src, h, w, y - 1, x), a02 = metric_at(src, h, w, y - 1, x + 1);
    const float a10 = metric_at(src, h, w, y, x - 1), a12 = metric_at(src, h, w, y, x + 1);
    const float a20 = metric_at(src, h, w, y + 1, x - 1), a21 = metric_at(src, h, w, y + 1, x), a22 = metric_at(src, h, w, y + 1, x + 1);
    const float gx = __fadd_rn(__fmul_rn(0.125f, __fadd_rn(__fsub_rn(a00, a02), __fsub_rn(a20, a22))), __fmul_rn(0.25f, __fsub_rn(a10, a12)));
    const float gy = __fadd_rn(__fmul_rn(0.125f, __fadd_rn(__fsub_rn(a00, a20), __fsub_rn(a02, a22))), __fmul_rn(0.25f, __fsub_rn(a01, a21)));
    s += (double)__fadd_rn(fabsf(gx), fabsf(gy));
  }
  if (dst) {
    const int h2 = h >> 1, w2 = w >> 1;
    for (unsigned i = first; i < (unsigned)h2 * (unsigned)w2; i += step) {
      const float* r0 = src + (size_t)(2 * (i / (unsigned)w2)) * w + 2 * (i % (unsigned)w2);
      dst[i] = __fmul_rn(0.25f, __fadd_rn(__fadd_rn(r0[0], r0[1]), __fadd_rn(r0[w], r0[w + 1])));
    }
  }
  return s;
}
// small: plane blockIdx.x, everything in LDS (h * w <= kMetricLanesLdsN, so level l holds at most kMetricLanesLdsN >> 2 l values)
__global__ __launch_bounds__(256) void metric_lanes_small_kernel(const MetricLanesParams p) {
  __shared__ float d0[kMetricLanesLdsN];
  __shared__ float pool[kMetricLanesLdsN / 4 + kMetricLanesLdsN / 16 + kMetricLanesLdsN / 64 + kMetricLanesLdsN / 256];
  __shared__ double lds[256];
  const int c = blockIdx.x, t = threadIdx.x;
  const int ch = (p.h + 1) >> 1, cw = (p.w + 1) >> 1;
  double bce = 0.0;
  unsigned bad = 0;
  for (int i = t; i < ch * cw; i += 256) metric_lanes_cell(p, c, i / cw, i % cw, d0, pool, &bce, &bad);
  bce = metric_block_reduce(bce, lds, MetricSumJoin());   // its barriers also publish d0 and level 1
  const double nbad = metric_block_reduce((double)bad, lds, MetricSumJoin());
  if (t == 0) {
    *metric_lanes_part(p, c, 0) = bce;
    *metric_lanes_part(p, c, 6) = nbad;
  }
  double e = metric_lanes_edge_part(d0, p.h, p.w, nullptr, (unsigned)t, 256u);
  e = metric_block_reduce(e, lds, MetricSumJoin());
  if (t == 0) *metric_lanes_part(p, c, 1) = e;
  float* src = pool;
  int h = p.h >> 1, w = p.w >> 1;
  for (int s = 1; s < 5; ++s) {   // level s + 1 is written behind level s while that is read; the reduction's barriers publish it
    float* dst = src + (size_t)h * w;
    e = metric_lanes_edge_part(src, h, w, s < 4 ? dst : (float*)nullptr, (unsigned)t, 256u);
    e = metric_block_reduce(e, lds, MetricSumJoin());
    if (t == 0) *metric_lanes_part(p, c, 1 + s) = e;
    src = dst;
    h >>= 1;
    w >>= 1;
  }
}
// general, launch 1: grid (nb, 3); D0 and level 1 into scratch, the BCE and non-finite partials
__global__ __launch_bounds__(256) void metric_lanes_prep_kernel(const MetricLanesParams p, unsigned pooled_elems) {
  __shared__ double lds[256];
  const int c = blockIdx.y;
  const unsigned ch = (unsigned)(p.h + 1) >> 1, cw = (unsigned)(p.w + 1) >> 1;
  float* d0 = p.d0 + (size_t)c * p.h * p.w;
  float* p1 = p.pooled + (size_t)c * pooled_elems;
  double bce = 0.0;
  unsigned bad = 0;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < ch * cw; i += gridDim.x * 256) metric_lanes_cell(p, c, (int)(i / cw), (int)(i % cw), d0, p1, &bce, &bad);
  bce = metric_block_reduce(bce, lds, MetricSumJoin());
  const double nbad = metric_block_reduce((double)bad, lds, MetricSumJoin());
  if (threadIdx.x == 0) {
    metric_lanes_part(p, c, 0)[blockIdx.x] = bce;
    metric_lanes_part(p, c, 6)[blockIdx.x] = nbad;
  }
}
// general, launches 2 .. 6: grid (nb, 3); scale s of plane blockIdx.y, src and dst planes `src_stride` / `dst_stride` floats apart
__global__ __launch_bounds__(256) void metric_lanes_edge_kernel(const MetricLanesParams p, int s, const float* src, size_t src_stride, int h, int w, float* dst, size_t dst_stride) {
  __shared__ double lds[256];
  const int c = blockIdx.y;
  double e = metric_lanes_edge_part(src + c * src_stride, h, w, dst ? dst + c * dst_stride : (float*)nullptr, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
  e = metric_block_reduce(e, lds, MetricSumJoin());
  if (threadIdx.x == 0) metric_lanes_part(p, c, 1 + s)[blockIdx.x] = e;
}
// the record: partials folded in the fixed tree (nb[0] prep workgroups, nb[1 + s] of scale s; all 1 behind the small kernel), every mean one fp32 division of
// the double sum rounded to fp32, then the trainer's fp32 expressions: edge_c = ((((e0 + e1) + e2) + e3) + e4) / 5, loss_c = edge_c + bce_c, score = (2 l0 + 2 l1) + l2
struct MetricLanesFinish {
  unsigned nb[6], n_edge[5];
};
__global__ __launch_bounds__(256) void metric_lanes_finish_kernel(const MetricLanesParams p, const MetricLanesFinish f) {
  __shared__ double lds[256];
  const unsigned t = threadIdx.x, n = (unsigned)p.h * (unsigned)p.w;
  LanesRecord r;
  double bad = 0.0;
  for (int c = 0; c < 3; ++c) {
    double v[kLanesParts];
    for (int k = 0; k < kLanesParts; ++k) {
      const unsigned nb = (k == 0 || k == 6) ? f.nb[0] : f.nb[k];
      v[k] = nb == 1 ? metric_lanes_part(p, c, k)[0] : metric_block_reduce(t < nb ? metric_lanes_part(p, c, k)[t] : 0.0, lds, MetricSumJoin());   // nb is uniform
    }
    bad += v[6];
    r.bce[c] = __fdiv_rn((float)v[0], (float)n);
    float e = 0.0f;
    for (int s = 0; s < 5; ++s) {
      r.edge[c][s] = __fdiv_rn((float)v[1 + s], (float)f.n_edge[s]);
      e = s ? __fadd_rn(e, r.edge[c][s]) : r.edge[c][s];
    }
    r.loss[c] = __fadd_rn(__fdiv_rn(e, 5.0f), r.bce[c]);
  }
  if (t != 0) return;
  r.score = __fadd_rn(__fadd_rn(__fmul_rn(2.0f, r.loss[0]), __fmul_rn(2.0f, r.loss[1])), r.loss[2]);
  r.n = n;
  r.nonfinite = (unsigned)bad;
  if (r.nonfinite) {
    const float nan = __uint_as_float(0x7FC00000u);
    for (int c = 0; c < 3; ++c) {
      r.bce[c] = r.loss[c] = nan;
      for (int s = 0; s < 5; ++s) r.edge[c][s] = nan;
    }
    r.score = nan;
  }
  *p.rec = r;
}

size_t metric_lanes_pooled_elems(int h, int w) {
  size_t t = 0;
  for (int s = 0; s < 4; ++s) {
    h >>= 1;
    w >>= 1;
    t += (size_t)h * w;
  }
  return t;
}
hipError_t launch_metric_lanes(const MetricLanesParams& p, hipStream_t st) {
  if (!p.logits || !p.gt || !p.part || !p.rec || p.h < kMetricLanesMinSide || p.w < kMetricLanesMinSide || (long long)p.h * p.w > (long long)kMetricLanesMaxN ||
      p.gt_form < kLanesGtPlanes || p.gt_form > kLanesGtRef || (reinterpret_cast<uintptr_t>(p.logits) & 3) ||
      (p.gt_form != kLanesGtBits && (reinterpret_cast<uintptr_t>(p.gt) & 3)))
    return hipErrorInvalidValue;
  const unsigned n = (unsigned)p.h * (unsigned)p.w;
  MetricLanesFinish f{};
  int h = p.h, w = p.w;
  for (int s = 0; s < 5; ++s) {
    f.n_edge[s] = (unsigned)h * (unsigned)w;
    h >>= 1;
    w >>= 1;
  }
  if (n <= kMetricLanesLdsN) {
    for (unsigned& b : f.nb) b = 1;
    hipLaunchKernelGGL(metric_lanes_small_kernel, dim3(3), dim3(256), 0, st, p);
    VP_LAUNCH(metric_lanes_finish_kernel, dim3(1), dim3(256), 0, st, p, f);
  }
  if (!p.d0 || !p.pooled) return hipErrorInvalidValue;
  const size_t pe = metric_lanes_pooled_elems(p.h, p.w);
  f.nb[0] = metric_blocks((size_t)((p.h + 1) >> 1) * (size_t)((p.w + 1) >> 1));
  hipLaunchKernelGGL(metric_lanes_prep_kernel, dim3(f.nb[0], 3), dim3(256), 0, st, p, (unsigned)pe);
  const float* src = p.d0;
  size_t src_stride = n;
  float* dst = p.pooled;
  h = p.h;
  w = p.w;
  for (int s = 0; s < 5; ++s) {
    f.nb[1 + s] = metric_blocks(f.n_edge[s]);
    if (s > 0) dst += (size_t)h * w;   // level s + 1 behind level s
    hipLaunchKernelGGL(metric_lanes_edge_kernel, dim3(f.nb[1 + s], 3), dim3(256), 0, st, p, s, src, src_stride, h, w, (s > 0 && s < 4) ? dst : (float*)nullptr, pe);
    if (s == 0) {
      src = p.pooled;
      src_stride = pe;
    } else {
      src = dst;
    }
    h >>= 1;
    w >>= 1;
  }
  VP_LAUNCH(metric_lanes_finish_kernel, dim3(1), dim3(256), 0, st, p, f);
}

// one line per workgroup (kernels.hpp: the summation order)
__global__ __launch_bounds__(256) void metric_rows_kernel(const MetricRowsParams p) {
  __shared__ double lds[256];
  const size_t o = (size_t)blockIdx.x * p.rows;
  double sd = 0.0, sc = 0.0, nv = 0.0, nt = 0.0;
  for (int r = threadIdx.x; r < p.rows; r += 256) {
    const float hv = p.hv[o + r], th = p.thv[o + r];
    const float m = hv > 0.5f ? 1.0f : 0.0f, mt = th > 0.5f ? 1.0f : 0.0f;
    sd += (double)fabsf(__fsub_rn(__fmul_rn(p.xp[o + r], m), __fmul_rn(p.txp[o + r], mt)));
    sc += (double)hv;
    nv += (double)m;
    nt += (double)mt;
  }
  sd = metric_block_reduce(sd, lds, MetricSumJoin());
  sc = metric_block_reduce(sc, lds, MetricSumJoin());
  nv = metric_block_reduce(nv, lds, MetricSumJoin());
  nt = metric_block_reduce(nt, lds, MetricSumJoin());
  if (threadIdx.x != 0) return;
  RowsRecord r;
  r.dist = (float)(sd / (double)p.rows);
  r.conf = (float)(sc / (double)p.rows);
  r.tp = 0;
  for (int k = 0; k < p.n_thr; ++k) r.tp |= ((double)r.dist < p.thr[k] ? 1u : 0u) << k;   // in double against the fp32 value, as .item() compares
  r.valid = (unsigned)nv;
  r.target_valid = (unsigned)nt;
  p.rec[blockIdx.x] = r;
}
hipError_t launch_metric_rows(const MetricRowsParams& p, hipStream_t st) {
  if (!p.xp || !p.hv || !p.txp || !p.thv || !p.rec || p.n_lines < 1 || p.n_lines > kMetricRowsMaxLines || p.rows < 1 || p.rows > kMetricRowsMaxRows || p.n_thr < 1 ||
      p.n_thr > kMetricRowsMaxThr)
    return hipErrorInvalidValue;
  VP_LAUNCH(metric_rows_kernel, dim3(p.n_lines), dim3(256), 0, st, p);
}

// ------------------------------------------------------------------------------------------ vp_metric, label part
// load_data_scene_seg.py:55-166 (extractROI, createGroundTruth), load_data_scene_3d.py:59-66 and the nearest resize behind them, restated (kernels.hpp).
// the class of a colour: the first table row it equals; 3: none
__device__ __forceinline__ unsigned label_class(const LabelSegParams& p, unsigned rgb) {
  unsigned c = 3u;
  for (int k = p.n_colours - 1; k >= 0; --k) c = rgb == p.rgb[k] ? (unsigned)p.cls[k] : c;
  return c;
}
// one pixel of the crop into cnt = freq[3], unmatched (colour) or cnt[0] = nonzero (mask)
__device__ __forceinline__ void label_count(const LabelSegParams& p, unsigned v, unsigned* cnt) {
  if (p.channels == 3) {
    const unsigned c = label_class(p, v);
    cnt[0] += c == 0u;
    cnt[1] += c == 1u;
    cnt[2] += c == 2u;
    cnt[3] += c == 3u;
  } else {
    cnt[0] += v != 0u;
  }
}
// The part [y0, y0 + ih) x [x0, x0 + iw) of the crop that lies inside the image, in runs of 16 pixels per row: a full run that starts on a 16-byte
// boundary is read with 16-byte loads (every run of a row when the stride and the row's first byte are multiples of 16, as for a 1920-wide label),
// any other run byte by byte.  Counters per work-item, a shuffle fold per wave, one partial per workgroup.
__global__ __launch_bounds__(256) void label_stats_kernel(const LabelSegParams p, int x0, int y0, int iw, int ih) {
  __shared__ unsigned wave_cnt[4][4];
  unsigned cnt[4] = {0u, 0u, 0u, 0u};
  const unsigned rpr = ((unsigned)iw + 15u) >> 4, total = rpr * (unsigned)ih;   // at most 1024 * 16384
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const unsigned row = i / rpr, run = i - row * rpr;
    const int x = x0 + (int)(run << 4);
    const int npx = min(16, x0 + iw - x);
    const uint8_t* src = p.label + (size_t)(y0 + (int)row) * (size_t)p.stride + (size_t)x * (size_t)p.channels;
    if (npx == 16 && !(reinterpret_cast<uintptr_t>(src) & 15)) {
      if (p.channels == 3) {
        unsigned w[12];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int4 q = reinterpret_cast<const int4*>(src)[k];
          w[4 * k] = (unsigned)q.x;
          w[4 * k + 1] = (unsigned)q.y;
          w[4 * k + 2] = (unsigned)q.z;
          w[4 * k + 3] = (unsigned)q.w;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int word = (24 * j) >> 5, sh = (24 * j) & 31;
          unsigned v = w[word] >> sh;
          if (sh > 8) v |= w[word + 1] << (32 - sh);   // sh is 0, 8, 16 or 24: word + 1 <= 11 whenever sh > 8
          label_count(p, v & 0xFFFFFFu, cnt);
        }
      } else {
        const int4 q = *reinterpret_cast<const int4*>(src);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const unsigned w = (unsigned)((j >> 2) == 0 ? q.x : (j >> 2) == 1 ? q.y : (j >> 2) == 2 ? q.z : q.w);
          label_count(p, (w >> (8 * (j & 3))) & 255u, cnt);
        }
      }
    } else {
      for (int j = 0; j < npx; ++j) {
        const uint8_t* s = src + j * p.channels;
        label_count(p, p.channels == 3 ? ((unsigned)s[0] | (unsigned)s[1] << 8 | (unsigned)s[2] << 16) : (unsigned)s[0], cnt);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt[k] += __shfl_xor(cnt[k], o);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) wave_cnt[threadIdx.x >> 6][k] = cnt[k];
  }
  __syncthreads();
  if (threadIdx.x < 4) p.part[4 * blockIdx.x + threadIdx.x] = wave_cnt[0][threadIdx.x] + wave_cnt[1][threadIdx.x] + wave_cnt[2][threadIdx.x] + wave_cnt[3][threadIdx.x];
}
struct LabelAddJoin {
  __device__ __forceinline__ unsigned operator()(unsigned a, unsigned b) const { return a + b; }
};
// one work-item per output pixel; workgroup 0 also folds the stats partials (nb <= 256) and stores the record.  outside: crop pixels outside the image,
// black_cls: the class of (0, 0, 0) by the table (3: none) -- they are counted in it
__global__ __launch_bounds__(256) void label_gt_kernel(const LabelSegParams p, unsigned nb, unsigned outside, unsigned black_cls) {
  __shared__ unsigned lds[256];
  const unsigned n_out = (unsigned)p.oh * (unsigned)p.ow, i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_out) {
    const unsigned oy = i / (unsigned)p.ow, ox = i - oy * (unsigned)p.ow;
    const int sy = p.t + p.ty[oy], sx = p.l + p.tx[ox];
    unsigned v = 0u;
    if (sy >= 0 && sy < p.h && sx >= 0 && sx < p.w) {
      const uint8_t* s = p.label + (size_t)sy * (size_t)p.stride + (size_t)sx * (size_t)p.channels;
      v = p.channels == 3 ? ((unsigned)s[0] | (unsigned)s[1] << 8 | (unsigned)s[2] << 16) : (unsigned)s[0];
    }
    if (p.channels == 3) {
      const unsigned c = label_class(p, v);
      v = c < 3u ? c : 255u;
    }
    p.gt[i] = (uint8_t)v;
  }
  if (blockIdx.x != 0) return;
  unsigned tot[4];
  for (int k = 0; k < 4; ++k) tot[k] = metric_block_reduce(threadIdx.x < nb ? p.part[4 * threadIdx.x + k] : 0u, lds, LabelAddJoin());
  if (threadIdx.x != 0) return;
  LabelRecord r;
  r.kind = p.channels == 3 ? 0 : 2;
  r.n = (unsigned)p.cw * (unsigned)p.ch;
  for (int k = 0; k < 3; ++k) r.freq[k] = tot[k] + (p.channels == 3 && black_cls == (unsigned)k ? outside : 0u);
  r.unmatched = p.channels == 3 ? tot[3] : 0u;
  r.outside = outside;
  r.nonfinite = 0u;
  r.mn = r.mx = 0.0;
  *p.rec = r;
}
hipError_t launch_label_seg(const LabelSegParams& p, hipStream_t st) {
  if (!p.label || !p.ty || !p.tx || !p.gt || !p.part || !p.rec || (p.channels != 1 && p.channels != 3) || p.h < 1 || p.w < 1 || p.h > kLabelMaxSide || p.w > kLabelMaxSide ||
      (long long)p.stride < (long long)p.w * p.channels || p.cw < 1 || p.ch < 1 || p.l < kLabelCropMin || p.t < kLabelCropMin || (long long)p.l + p.cw > kLabelCropMax ||
      (long long)p.t + p.ch > kLabelCropMax || p.oh < 1 || p.ow < 1 || (long long)p.oh * p.ow > (long long)kMetricMaxN)
    return hipErrorInvalidValue;
  unsigned black_cls = 3u;
  if (p.channels == 3) {
    if (p.n_colours < 1 || p.n_colours > kLabelMaxColours) return hipErrorInvalidValue;
    for (int k = p.n_colours - 1; k >= 0; --k) {
      if (p.cls[k] > 2 || p.rgb[k] > 0xFFFFFFu) return hipErrorInvalidValue;
      if (p.rgb[k] == 0u) black_cls = p.cls[k];
    }
  }
  const int x0 = p.l > 0 ? p.l : 0, y0 = p.t > 0 ? p.t : 0;
  const int x1 = p.l + p.cw < p.w ? p.l + p.cw : p.w, y1 = p.t + p.ch < p.h ? p.t + p.ch : p.h;
  const int iw = x1 > x0 ? x1 - x0 : 0, ih = y1 > y0 ? y1 - y0 : 0;
  const unsigned inside = (iw && ih) ? (unsigned)iw * (unsigned)ih : 0u, outside = (unsigned)p.cw * (unsigned)p.ch - inside;
  const unsigned nb = metric_blocks(inside ? (size_t)((iw + 15) >> 4) * (size_t)ih : 0);
  hipLaunchKernelGGL(label_stats_kernel, dim3(nb), dim3(256), 0, st, p, x0, y0, inside ? iw : 0, inside ? ih : 0);
  VP_LAUNCH(label_gt_kernel, dim3(nblk((long long)p.oh * p.ow)), dim3(256), 0, st, p, nb, outside, black_cls);
}

// numpy's min and max of a plane: a NaN anywhere makes both NaN (the consumer applies that: `nan`).  Among equal values -0.0 is the smaller: numpy leaves
// the sign of a zero extreme to its reduction order, this does not.
struct LabelExtJoin {
  __device__ __forceinline__ LabelExtPartial operator()(const LabelExtPartial& a, const LabelExtPartial& b) const {
    LabelExtPartial r;
    r.mn = (b.mn < a.mn || (b.mn == a.mn && __builtin_signbit(b.mn))) ? b.mn : a.mn;
    r.mx = (b.mx > a.mx || (b.mx == a.mx && !__builtin_signbit(b.mx))) ? b.mx : a.mx;
    r.bad = a.bad + b.bad;
    r.nan = a.nan + b.nan;
    return r;
  }
};
__device__ __forceinline__ double label_depth_at(const LabelDepthParams& p, int y, int x) {
  const size_t i = (size_t)y * (size_t)p.stride + (size_t)x;
  return p.dtype == kLabelF64 ? static_cast<const double*>(p.label)[i] : (double)static_cast<const float*>(p.label)[i];   // fp32 -> fp64 is exact
}
// rows in turn over the workgroups, a row's elements over the work-items: one partial per workgroup
__global__ __launch_bounds__(256) void label_minmax_kernel(const LabelDepthParams p) {
  __shared__ LabelExtPartial lds[256];
  LabelExtPartial s{INFINITY, -INFINITY, 0u, 0u};
  for (int y = blockIdx.x; y < p.h; y += gridDim.x)
    for (int x = threadIdx.x; x < p.w; x += 256) {
      const double v = label_depth_at(p, y, x);
      if (v != v) {
        ++s.nan;
        ++s.bad;
      } else {
        s = LabelExtJoin()(s, LabelExtPartial{v, v, fabs(v) == (double)INFINITY ? 1u : 0u, 0u});
      }
    }
  s = metric_block_reduce(s, lds, LabelExtJoin());
  if (threadIdx.x == 0) p.part[blockIdx.x] = s;
}
// every workgroup folds the nb <= 256 partials (partial b through work-item b, the fixed tree), then one work-item per output pixel:
// g = (v - mn) / (mx - mn) in the label's type, one subtraction and one division, fp64 rounded to nearest into fp32
__global__ __launch_bounds__(256) void label_depth_gt_kernel(const LabelDepthParams p, unsigned nb) {
  __shared__ LabelExtPartial lds[256];
  LabelExtPartial s{INFINITY, -INFINITY, 0u, 0u};
  if (threadIdx.x < nb) s = p.part[threadIdx.x];
  s = metric_block_reduce(s, lds, LabelExtJoin());
  const double mn = s.nan ? (double)NAN : s.mn, mx = s.nan ? (double)NAN : s.mx;
  const unsigned n_out = (unsigned)p.oh * (unsigned)p.ow, i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_out) {
    const unsigned oy = i / (unsigned)p.ow, ox = i - oy * (unsigned)p.ow;
    const size_t at = (size_t)p.ty[oy] * (size_t)p.stride + (size_t)p.tx[ox];
    float g;
    if (p.dtype == kLabelF64) {
      g = (float)((static_cast<const double*>(p.label)[at] - mn) / (mx - mn));
    } else {
      const float fmn = (float)mn, fmx = (float)mx;   // exact: both are fp32 values of the plane
      g = __fdiv_rn(__fsub_rn(static_cast<const float*>(p.label)[at], fmn), __fsub_rn(fmx, fmn));
    }
    p.gt[i] = g;
  }
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  LabelRecord r;
  r.kind = 1;
  r.n = (unsigned)p.h * (unsigned)p.w;
  r.freq[0] = r.freq[1] = r.freq[2] = r.unmatched = r.outside = 0u;
  r.nonfinite = s.bad;
  r.mn = mn;
  r.mx = mx;
  *p.rec = r;
}
hipError_t launch_label_depth(const LabelDepthParams& p, hipStream_t st) {
  if (!p.label || !p.ty || !p.tx || !p.gt || !p.part || !p.rec || (p.dtype != kLabelF32 && p.dtype != kLabelF64) || p.h < 1 || p.w < 1 || p.h > kLabelMaxSide ||
      p.w > kLabelMaxSide || p.stride < p.w || p.oh < 1 || p.ow < 1 || (long long)p.oh * p.ow > (long long)kMetricMaxN ||
      (reinterpret_cast<uintptr_t>(p.label) & (p.dtype == kLabelF64 ? 7 : 3)))
    return hipErrorInvalidValue;
  const unsigned nb = p.h < kMetricBlocks ? (unsigned)p.h : (unsigned)kMetricBlocks;
  hipLaunchKernelGGL(label_minmax_kernel, dim3(nb), dim3(256), 0, st, p);
  VP_LAUNCH(label_depth_gt_kernel, dim3(nblk((long long)p.oh * p.ow)), dim3(256), 0, st, p, nb);
}

}  // namespace vp

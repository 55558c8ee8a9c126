// Kernel parameter blocks + host launchers of libvp_hip (definitions in kernels_conv.hip / kernels_misc.hip).
#pragma once
#include "common.hpp"

namespace vp {

// developer option set through vp_set_option (options.cpp), or nullptr -- the library never reads the environment
const char* dev_option(const char* key);
bool dev_option_is(const char* key, char first);  // value set and starting with `first`: one lookup

struct PreprocessParams {
  const uint8_t* frame;  // device, HxWx3
  int stride;            // bytes per row
  const int* xtab;       // [out_w][4] = x0, x1, a0, a1
  const int* ytab;       // [out_h][4] = y0, y1, b0, b1
  int out_h, out_w;
  int src_c[3];          // source byte index feeding output plane 0,1,2
  float mean[3], stdv[3];
  float* out;            // [3][out_h][out_w]
  int norm_form;         // 0: q / 255 (torchvision to_tensor), 1: q * fl(1/255) (cv::Mat::convertTo) -- kernels_misc.hip unit_from_u8
};

// Pillow's antialiased resample (PIL.Image.resize with BILINEAR / BICUBIC; src/libImaging/Resample.c 8bpc path) + /255 + (x-mean)/std +
// HWC->CHW: the AutoDrive frame path (Models/visualizations/AutoDrive/video_visualization.py:29-33) and the scene networks' Python
// visualisation scripts.  Definition pinned against PIL itself: oracle/pre_post.py resize_pil_u8.  Two passes, as Pillow's: horizontal
// into a u8 image [in_h][out_w][3], vertical from it; coefficient tables (22 fractional bits) are built on the host in double.
struct PilResampleParams {
  const uint8_t* frame;  // device, in_h x in_w x 3
  int stride;            // bytes per row
  int in_h, in_w, out_h, out_w;
  const int* hb;         // [out_w][2] = first source column, tap count
  const int* hk;         // [out_w][hks]
  int hks;
  const int* vb;         // [out_h][2]
  const int* vk;         // [out_h][vks]
  int vks;
  uint8_t* tmp;          // [in_h][out_w][3]
  int src_c[3];
  float mean[3], stdv[3];
  float* out;            // [3][out_h][out_w]
  int norm_form;         // as PreprocessParams
};

// vp_frame (include/vp_hip.h): a camera frame in its native format -> packed BGR8 on the device, once, behind the upload.  kernels_misc.hip
// frame_to_bgr8_kernel.  format: the vp_frame_format code.  p0 / s0: the first plane (the 4:2:0 formats: the Y plane) and its row stride in bytes;
// p1 / s1: NV12's interleaved UV plane, NV21's VU plane, I420's U plane, YV12's V plane; p2 / s2: I420's V plane, YV12's U plane (the planes in the
// format's own order: the launcher hands the kernel YV12 as I420 with the two chroma planes exchanged).  dst rows are dst_pitch = 12 * ceil(w / 4)
// bytes apart (== 3 * w when w is a multiple of 4): one work-item stores the three words of four pixels, bytes behind the last pixel of a row are
// written as 0.
// Format codes 0 .. 7 and 16 .. 18 (8 .. 15 stay unknown); frame_format_index: their dense index for tables, -1 for anything else.
constexpr int kFrameFormats = 11;   // BGR8, RGB8, BGRA8, RGBA8, GRAY8, NV12, YUY2, UYVY, I420, YV12, NV21
inline int frame_format_index(int format) { return format >= 0 && format < 8 ? format : (format >= 16 && format <= 18 ? format - 8 : -1); }
inline bool frame_format_420(int format) { return format == 5 || (format >= 16 && format <= 18); }   // one (U, V) per 2x2 block
inline bool frame_format_planar(int format) { return format == 16 || format == 17; }                // three planes
inline int frame_bgr_pitch(int w) { return 12 * ((w + 3) / 4); }
// The colour standards (include/vp_hip.h vp_color_matrix x vp_color_range), 20 fractional bits.  ONE table, color_standard() below; both kernels take
// their constants from it as uniform parameters.
//   inverse:  y = cy * max(0, Y - off), u = U - 128, v = V - 128;  R = y + cvr v,  G = y - cvg v - cug u,  B = y + cub u
//   forward:  Y = yk . (R, G, B) + (off << 20),  U = uk . (R, G, B) + (128 << 20),  V = vk . (R, G, B) + (128 << 20)
// each + 2^19, arithmetic shift by 20, clamp to 0 .. 255.
struct YuvToBgr {
  int off, cy, cvr, cvg, cug, cub;
};
struct BgrToYuv {
  int off;
  int yk[3], uk[3], vk[3];   // R, G, B
};
struct ColorStandard {
  YuvToBgr inv;
  BgrToYuv fwd;
};
inline const ColorStandard& color_standard(int matrix, int range) {
  static const ColorStandard table[2][2] = {
      {{{16, 1220542, 1673527, 852492, 409993, 2116026}, {16, {269484, 528482, 102760}, {-155188, -305135, 460324}, {460324, -385875, -74448}}},     // BT.601 limited: OpenCV's
       {{0, 1048576, 1470104, 748826, 360853, 1858077}, {0, {313524, 615514, 119538}, {-176932, -347356, 524288}, {524288, -439026, -85262}}}},      // BT.601 full
      {{{16, 1220945, 1879825, 558796, 223607, 2215014}, {16, {191455, 644067, 65019}, {-105533, -355018, 460551}, {460551, -418321, -42230}}},      // BT.709 limited
       {{0, 1048576, 1651297, 490864, 196424, 1945738}, {0, {222927, 749942, 75707}, {-120138, -404150, 524288}, {524288, -476214, -48074}}}}};      // BT.709 full
  return table[matrix & 1][range & 1];
}
struct FrameToBgrParams {
  const uint8_t* p0;
  const uint8_t* p1;
  const uint8_t* p2;
  int s0, s1, s2;
  int h, w;
  int format;
  uint8_t* dst;
  int dst_pitch;
  YuvToBgr k;           // color_standard(matrix, range).inv; read by the YUV formats only
};
hipError_t launch_frame_to_bgr8(const FrameToBgrParams& p, hipStream_t st);

// The upload-only formats of vp_frame (include/vp_hip.h): 16-bit grey (20), P010 (21), raw Bayer in 8-bit (32 .. 35) and 16-bit (36 .. 39) containers.
// They have kernels of their own and no dense index: frame_format_index answers -1 for them, so the canvas and every table of kFrameFormats entries
// keep refusing them.  16-bit samples are little-endian words; their planes and strides are 2-byte aligned (checked at the upload).
inline bool frame_format_deep(int format) { return format == 20 || format == 21; }
inline bool frame_format_bayer(int format) { return format >= 32 && format <= 39; }
inline bool frame_format_bayer16(int format) { return format >= 36 && format <= 39; }
// frame_deep_to_bgr8_kernel: every 16-bit sample is narrowed first, x8 = min(255, (s + 128) >> 8) (MSB-aligned, as P010 / P012 / P016 are); from there
// P010 (Y words in p0, interleaved U V words in p1) is NV12's arithmetic and GRAY16 is GRAY8's, with their work-item shapes.
struct FrameDeepParams {
  const uint8_t* p0;
  const uint8_t* p1;
  int s0, s1;           // bytes
  int h, w;
  int format;           // 20 GRAY16, 21 P010
  uint8_t* dst;
  int dst_pitch;
  YuvToBgr k;           // read by P010 only
};
hipError_t launch_frame_deep_to_bgr8(const FrameDeepParams& p, hipStream_t st);
// frame_raw_to_bgr8_kernel: linearise, white balance, bilinear demosaic, optional matrix, tone -- include/vp_hip.h states the arithmetic as the
// DEFINITION.  One work-item produces a 4 x 2 block (two whole CFA cells) from its 6 x 4 sample window, read at mirrored addresses (-1 -> 1, n -> n - 2:
// CFA parity is kept and no index leaves the plane).  The CFA order is two bits: green00 (the site (0, 0) is green) and red_row0 (row 0 holds the red
// sites), so a site (y, x) is green when (x ^ y ^ green00) & 1, and otherwise red when (y & 1) != red_row0.  Everything but the samples is uniform
// over the launch.  lut: device memory, 1 << min(bits, 12) entries, or nullptr for the rounding shift to 8 bits.
struct FrameRawParams {
  const uint8_t* src;
  int stride;           // bytes
  int h, w;
  int wide;             // 1: 16-bit words, 0: bytes
  int green00, red_row0;
  int bits;             // B, the significant bits: 8, 10, 12, 14 or 16 (8 only with bytes, the others only with words)
  int shift, black;
  int gains[3];         // Q8; R, G, B
  int ccm_on;
  int ccm[9];           // Q10, rows and columns R, G, B
  const uint8_t* lut;
  uint8_t* dst;
  int dst_pitch;
};
hipError_t launch_frame_raw_to_bgr8(const FrameRawParams& p, hipStream_t st);

// vp_canvas (include/vp_hip.h): one BGR8 picture per camera frame with the geometry and pitch of a vp_frame's image (rows frame_bgr_pitch(w) apart, base and
// pitch multiples of 4), drawn into IN PLACE.  Every kernel below gives one work-item an aligned four-pixel block of a canvas row -- three 32-bit words
// in, three out -- and leaves the pixels of the block it does not own as it read them (a region's odd edge, the zero bytes behind a row's end).
// canvas_blend_kernel: viz_blend_kernel's label -> LUT -> 50/50 blend on the region (x0, y0, w, h) of the canvas; ytab [h] / xtab [w]: nearest tables
// of the region's size into the mh x mw label mask.
struct CanvasBlendParams {
  const uint8_t* mask;
  int mw;
  const int* ytab;
  const int* xtab;
  const uint8_t* lut;   // [256][3] BGR
  uint8_t* canvas;
  int pitch;
  int x0, y0, w, h;
};
hipError_t launch_canvas_blend(const CanvasBlendParams& p, int canvas_h, int canvas_w, hipStream_t st);
// canvas_boxes_kernel: up to kCanvasBoxChunk boxes per launch, walked IN ORDER by every work-item over its own pixels, so the result is the sequential
// one with one read and one write per pixel.  A box is the inclusive rectangle [x0, x1] x [y0, y1] before clipping (it may reach outside the canvas):
// its one-pixel outline takes the colour, its interior d = (colour + 4 d) / 5 rounded to nearest (never a tie).  ux / uy: the union of the clipped
// boxes, the pixels the launch visits.
constexpr int kCanvasBoxChunk = 64;
struct CanvasBox {
  int x0, y0, x1, y1;
  unsigned bgr;         // b | g << 8 | r << 16
};
struct CanvasBoxParams {
  uint8_t* canvas;
  int pitch;
  int ux0, uy0, ux1, uy1;
  int n;
  CanvasBox box[kCanvasBoxChunk];
};
hipError_t launch_canvas_boxes(const CanvasBoxParams& p, int canvas_h, int canvas_w, hipStream_t st);
// canvas_to_format_kernel: the inverse of frame_to_bgr8_kernel -- the same four-pixel blocks, row pairs for the 4:2:0 formats.  Chroma: of the even
// pixel (4:2:0: of the top-left pixel of the 2x2 block), or with chroma_mean the rounded mean of the group's per-pixel (clamped) samples, all of which
// the one work-item owns.  The planes are the canvas's own staging: rows canvas_plane_pitch(format, w, plane) apart, bytes behind a row's end zero up to
// the last block's store.  Plane 0 and the interleaved chroma plane are stored as whole words; a work-item's share of a planar chroma row is two bytes,
// stored as one aligned 16-bit value.  p1 / p2: as FrameToBgrParams, the format's own order.  BGR8 needs no kernel.  include/vp_hip.h vp_canvas_fetch.
inline int canvas_plane_pitch(int format, int w, int plane = 0) {
  static const int block_bytes[kFrameFormats] = {12, 12, 16, 16, 4, 4, 8, 8, 4, 4, 4};   // of four pixels, plane 0
  const int blocks = (w + 3) / 4;
  if (plane > 0 && frame_format_planar(format)) return (2 * blocks + 3) & ~3;
  return block_bytes[frame_format_index(format)] * blocks;
}
struct CanvasToFormatParams {
  const uint8_t* src;
  int src_pitch;
  int h, w;
  int format;
  uint8_t* p0;
  uint8_t* p1;          // 4:2:0: the second plane, rows dst_pitch_c apart
  uint8_t* p2;          // planar: the third plane, likewise
  int dst_pitch;        // canvas_plane_pitch(format, w)
  int dst_pitch_c;      // canvas_plane_pitch(format, w, 1)
  int chroma_mean;      // 0: the even pixel; 1: the mean of the group
  BgrToYuv k;           // color_standard(matrix, range).fwd
};
hipError_t launch_canvas_to_format(const CanvasToFormatParams& p, hipStream_t st);
// depth_colorize_kernel's value -> u8 -> table step, written into the region (x0, y0, w, h) of the canvas instead of a packed image; src: [h][w] fp32
hipError_t launch_canvas_depth(const float* src, const unsigned* mm, const uint8_t* lut, uint8_t* canvas, int pitch, int x0, int y0, int w, int h,
                               int canvas_h, int canvas_w, hipStream_t st);
// canvas_add_planes_kernel: the additive overlays of drawRawMasksInPlace (visualize.cpp:312-388) as ONE clamped sum per pixel.  planes: fp32
// [n_planes][mh][mw], plane_stride = mh * mw; ytab [h] / xtab [w]: nearest tables of the region's size into mh x mw, as CanvasBlendParams.  Every plane k
// with planes[k][my][mx] > threshold (fp32 compare: NaN is false) adds add[k] = b | g << 8 | r << 16 to the pixel, each channel min(255, d + sum): all
// increments are non-negative, so this equals the overlays applied one after the other, with one read and one write per pixel.
constexpr int kCanvasMaxPlanes = 4;
struct CanvasAddPlanesParams {
  const float* planes;
  int n_planes, plane_stride, mw;
  const int* ytab;
  const int* xtab;
  float threshold;
  unsigned add[kCanvasMaxPlanes];
  uint8_t* canvas;
  int pitch;
  int x0, y0, w, h;
};
hipError_t launch_canvas_add_planes(const CanvasAddPlanesParams& p, int canvas_h, int canvas_w, hipStream_t st);
// canvas_points_kernel: filled discs of one colour, dx * dx + dy * dy <= radius * radius around each point, clipped to the canvas.  Up to kCanvasPointChunk
// points per launch, walked by every work-item over its own block (one colour: the order does not matter).  ux / uy: the pixels the launch visits.
// rows == nullptr: the points are pt[0, n).  rows != nullptr (vp_canvas_draw_lane_rows): the kernel forms them itself from the AutoSteer engine's
// device logits rows[0, n) = xp, rows[n, 2n) = h_vector (n = 64 <= kCanvasPointChunk): row i counts when h_vector[i] >= 0.5f and the fp32 product
// xp[i] * 1024.0f lies inside (-1e8, 1e8) (NaN does not); it sits at x = ox + (int)product, y = oy + i * 511 / 63.
constexpr int kCanvasPointChunk = 64;
constexpr int kCanvasMaxRadius = 16;
struct CanvasPoint {
  int x, y;
};
struct CanvasPointParams {
  uint8_t* canvas;
  int pitch;
  int ux0, uy0, ux1, uy1;
  int n, radius;
  unsigned bgr;         // b | g << 8 | r << 16
  const float* rows;
  int ox, oy;           // rows != nullptr: the region's origin
  CanvasPoint pt[kCanvasPointChunk];
};
hipError_t launch_canvas_points(const CanvasPointParams& p, int canvas_h, int canvas_w, hipStream_t st);
// canvas_resize_kernel: the u8 integer bilinear of preprocess_kernel (the same device function, the same linear_taps_u8 tables: oracle/pre_post.py
// resize_bilinear_u8) from one BGR8 picture into another.  One work-item forms an aligned four-pixel block of a destination row and stores its three
// words; bytes behind the row's end are written as 0.  dst rows are dst_pitch >= frame_bgr_pitch(out_w) apart: a picture canvas_to_format_kernel takes.
struct CanvasResizeParams {
  const uint8_t* src;
  int src_pitch, src_h, src_w;
  const int* xtab;      // [out_w][4] = x0, x1, a0, a1
  const int* ytab;      // [out_h][4] = y0, y1, b0, b1
  uint8_t* dst;
  int dst_pitch, out_h, out_w;
};
hipError_t launch_canvas_resize(const CanvasResizeParams& p, hipStream_t st);
// The baseline JPEG of a BGR8 picture (include/vp_hip.h "the picture as a baseline JPEG" states the stream as the DEFINITION).  Three kernels:
//   jpeg_blocks_kernel: a workgroup of 256 takes kJpegMcusPerGroup MCUs of 16 x 16 pixels in raster order.  Load: work-item (MCU, row pair, four-pixel
//     block) reads its two rows through load_bgr4 and forms 8 luma samples and 2 mean chroma pairs by canvas_to_format_kernel's own device functions
//     (luma_of / chroma_of / chroma_mean4 with k = color_standard(BT.601, full).fwd); sources beyond the picture are clamped per plane (Y: row h - 1 /
//     column w - 1; chroma: row h / 2 - 1 / column w / 2 - 1).  The level-shifted samples go to LDS as int16 [block][8][8], blocks kJpegBlockPitch apart.
//     Row pass: one work-item per (block, row), in place.  Column pass behind a barrier: one work-item per (block, column) forms F, quantises by
//     q[table][row-major index] and puts the value at its zigzag position of a second LDS image; behind another barrier the image is copied out as
//     16-byte words.  coef: int16 [MCU][6][64], MCUs in raster order, so the blocks of one restart interval are contiguous.
//   jpeg_entropy_kernel<WRITE>: one restart interval per work-item, coded serially (a 64-bit bit accumulator; coefficients read as 16-byte words, the next
//     block's eight loaded ahead, a word of eight zeros skipped as a run; the entries copied into LDS by each workgroup of 64).  WRITE false: len[i] = the interval's stuffed byte count + 2 for the RST marker behind it (none behind the last).
//     WRITE true: the bytes at out + off[i], then the marker.  huff: [2][16] DC then [2][256] AC entries, code | length << 16.
//   jpeg_scan_kernel: ONE workgroup of 256 turns len[0, n) into its exclusive prefix sum in place and stores the total in *total (a pinned word).
constexpr int kJpegMcusPerGroup = 8;
constexpr int kJpegBlockPitch = 72;    // int16 elements between the LDS images of two blocks: 64 + 8, still 16-byte aligned
constexpr int kJpegHuffWords = 2 * 16 + 2 * 256;
struct JpegBlocksParams {
  const uint8_t* src;     // BGR8, rows src_pitch apart, every row readable up to 12 * ceil(w / 4) bytes
  int src_pitch, h, w;    // h, w even
  int mcus_x, n_mcus;
  BgrToYuv k;             // color_standard(VP_COLOR_BT601, VP_COLOR_RANGE_FULL).fwd, whatever the canvas's own setting
  uint8_t q[2][64];       // luminance, chrominance; row-major
  int16_t* coef;          // [n_mcus][6][64], zigzag order
};
hipError_t launch_jpeg_blocks(const JpegBlocksParams& p, hipStream_t st);
struct JpegEntropyParams {
  const int16_t* coef;
  const uint32_t* huff;   // kJpegHuffWords entries on the device
  int n_mcus, restart_mcus, n_intervals;
  uint32_t* len;          // [n_intervals]: written by the counting launch, scanned in place, read by the writing launch as offsets
  uint8_t* out;           // the scan data (writing launch)
};
hipError_t launch_jpeg_entropy(const JpegEntropyParams& p, bool write, hipStream_t st);
hipError_t launch_jpeg_scan(uint32_t* len, int n, uint32_t* total, hipStream_t st);
// frame_remap_kernel: one BGR8 picture resampled through a per-pixel map (vp_frame's rectification: undistort, warp to the standard pose; include/vp_hip.h
// states the sample as the DEFINITION).  A map entry is (X, Y), the source coordinates of a destination pixel in units of 1/32 pixel, both inside
// [-2^20, 2^20 - 1]: ix = X >> 5, fx = X & 31 (likewise y); taps (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1) with the weights (32 - fx)(32 - fy),
// fx (32 - fy), (32 - fx) fy, fx fy; out = (sum w p + 512) >> 10 per channel.  border 0 (CONSTANT): a tap outside the source contributes 0; border 1
// (REPLICATE): tap coordinates are clamped to the picture.  Either way the addresses read are the clamped ones: no map value reads outside the source.
// The map is row-major with rows map_pitch = frame_remap_map_pitch(out_w) entries apart (a multiple of 4, base 16-byte aligned), so that one work-item
// reads the entries of its four pixels as two aligned 16-byte loads; it stores the three words of the block, bytes behind the row's end as 0.
// src rows are src_pitch >= 3 * src_w bytes apart and are read byte by byte.
struct RemapEntry {
  int x, y;
};
inline int frame_remap_map_pitch(int out_w) { return 4 * ((out_w + 3) / 4); }
struct FrameRemapParams {
  const uint8_t* src;
  int src_pitch, src_h, src_w;
  const RemapEntry* map;   // [out_h][map_pitch]
  int map_pitch;
  int border;              // 0 CONSTANT (value 0), 1 REPLICATE
  uint8_t* dst;
  int dst_pitch, out_h, out_w;
};
hipError_t launch_frame_remap(const FrameRemapParams& p, hipStream_t st);

struct StemParams {
  const float* in;  // [3][H][W]
  int H, W;         // input size (output is H/2 x W/2)
  const float* w;   // [27][32]  (k = (ci*3+ky)*3+kx, co fastest), BN scale folded
  const float* b;   // [32]
  ActView out;      // C = 32
  unsigned long long* zero;  // optional: the squeeze-excite accumulators of the frame, zeroed here (every block's pool comes later)
  size_t zero_n;
  int scaled;        // VP_ACT_SCALE: != 0 -> the result is stored times out_mul (2^-s_out); 0: out_mul is not read
  float out_mul;
};

struct DwParams {
  ActView in, out;
  const float* w;  // [k*k][C]
  const float* b;  // [C]
  int k, stride;
  // squeeze-excite average pool, fused: per-channel sums of the OUTPUT accumulated as 2^24 fixed-point int64
  // (integer atomics are associative -> bit-deterministic regardless of workgroup order); zeroed once per frame
  unsigned long long* sums;  // [replicas][C]
  int replicas;              // power of two <= kSeMaxReplicas: workgroup x-index & (replicas-1) picks the row
  // batched encoder (frames > 1): grid.z = frame; tensors are [frames][H][W][C], sums [frames][replicas][C]
  int frames;
};

// MBConv front half in one launch (kernels_mbconv.hip): expand 1x1 + SiLU -> depthwise k x k / stride + SiLU -> SE pool sums
struct MbFrontParams {
  ActView in;           // block input, H x W x Cin_pad, (hi, lo)
  const half_t* w_hi;   // expand weights [Cexp_pad][Cin_pad], BN folded, (hi, lo); zero rows / columns in the padding
  const half_t* w_lo;
  const float* b_exp;   // [Cexp_pad]
  const float* s_exp;   // [Cexp_pad] 2^-prescale of the expand weight rows (see ConvGemmParams::wscale)
  const float* w_dw;    // [k*k][Cexp_pad] fp32, BN folded
  const float* b_dw;    // [Cexp_pad]
  ActView out;          // H/stride x W/stride x Cexp_pad, (hi, lo)
  int k, stride;
  unsigned long long* sums;  // [replicas][Cexp_pad] fixed-point channel sums (as DwParams); may be null when zsums is given
  int replicas;
  // optional: the squeeze FC of the block's squeeze-excite, taken here from the workgroup's own channel sums (it is linear in them):
  // zsums[replica][j] += fixed(sum_c w1[j][c] * patch_sum[c]) -- the back half (mbconv_back) then starts from sq numbers, not from the means
  const float* w1;            // [sq][Cexp_pad] or null
  int sq;
  unsigned long long* zsums;  // [replicas][64] 2^24 fixed point
};

struct PoolParams {
  ActView in;
  float* partial;  // [nslab][C]
  int nslab;
};

struct SeParams {
  const unsigned long long* sums;  // [replicas][C] fixed-point channel sums of the fused pool (see DwParams)
  int replicas;
  int C, Creal, sq;
  float inv_hw;
  const float* w1;  // [sq][C]   (zero in pad columns)
  const float* b1;  // [sq]
  int frames;       // batched encoder: grid.y = frame; sums [frames][replicas][C]
};

struct ScaleWParams {
  const float* w;   // [rows][C] fp32 projection weights (BN folded)
  half_t* out_hi;   // [rows][C] = w * gate[c], (hi, lo) split
  half_t* out_lo;   // may be null
  int rows, C;
  const float* w2;  // [C][sq]  excite FC: gate[c] = sigmoid(b2[c] + w2[c][:] . s1)
  const float* b2;  // [C]
  int sq, Creal;
  int frames;       // batched encoder: grid.y = frame; out_hi / out_lo [frames][rows][C]
};

// MBConv back half in one launch (kernels_mbconv.hip): squeeze-excite gate -> projection 1x1 (+BN) with the gate folded into its K axis
// (+ residual).  One frame per pass, (hi, lo) activations.
struct MbBackParams {
  ActView in;          // depthwise output, H x W x C (hi, lo)
  SeParams se;         // pool sums of that tensor, squeeze FC (frames == 1, se.C == in.C)
  const unsigned long long* zsums;  // [se.replicas][64] pre-activation squeeze sums from mbconv_front (MbFrontParams::zsums), or null: means + FC here
  const float* w2q;    // excite FC as [sqp / 4][C][4]: w2q[(q * C + c) * 4 + i] = fc2.weight[c][4 q + i], zero beyond sq
  const float* b2;     // [C]
  int sqp;             // sq rounded up to a multiple of 4
  const float* w;      // [out.C][C] fp32 projection weights (BN folded) TIMES the row's power-of-two prescale, zero rows / columns in the padding
  const float* bias;   // [out.C]
  const float* wscale; // [out.C] 2^-prescale (see ConvGemmParams::wscale)
  ActView res;         // residual (the block's input, same geometry as out) or hi == nullptr
  ActView out;         // H x W x Cout_pad (hi, lo)
};

// AutoSpeed detector pre / post-processing (kernels_detect.hip; autospeed/onnxruntime_engine.cpp:71-113, :170-290).
struct LetterboxParams {
  const uint8_t* frame;  // device, h x w x 3 BGR
  int stride;            // bytes per row
  const int* xtab;       // [new_w][4] bilinear taps of the resize to new_w x new_h (as PreprocessParams)
  const int* ytab;       // [new_h][4]
  int new_w, new_h, pad_x, pad_y;
  int out_h, out_w;
  float* out;            // [3][out_h][out_w] planes R, G, B in [0, 1]; 114 / 255 outside the pasted image
};

struct Detection {       // == autoware_pov::vision::autospeed::Detection (detection.hpp:8-12) == vp_detection
  float x1, y1, x2, y2, confidence;
  int class_id;
};

// Decode + NMS, one kernel with two rules (kernels_detect.hip detect_nms_kernel).  kDetectPerClass: the C++ engines' postProcess + applyNMS.
// kDetectAgnostic: the Python wrapper's (Models/inference/auto_speed_infer.py:63-83, :100-106; vp_detect_postprocess_agnostic / _infer_pil):
// score = max over the classes of sigmoid(raw score), class = the first maximum, `score > conf` kept, greedy suppression at IoU > iou whatever the
// classes on the corner boxes in LETTERBOX pixels (the torchvision.ops.nms rule); only the kept boxes go (x - pad) / scale and are clamped to the frame.
enum DetectRule { kDetectPerClass = 0, kDetectAgnostic = 1 };
struct DetectParams {
  const float* raw;      // [num_attrs][num_boxes]: cx, cy, w, h (letterbox pixels), then the class scores
  int num_attrs, num_boxes;
  float conf_thresh, iou_thresh;
  float scale;           // letterbox geometry of the frame the tensor came from
  int pad_x, pad_y, orig_w, orig_h;
  float* boxes;          // scratch [num_boxes][4]: candidate boxes in sorted order
  int* cls;              // scratch [num_boxes]
  Detection* out;        // [out_cap] rows of 24 bytes: a Detection; under kDetectAgnostic six floats (class_id holds the class as a float's bits)
  int out_cap;
  int* count;            // [2]: detections kept (may exceed out_cap: only out_cap are written), candidates above the threshold
};
constexpr int kDetectMaxBoxes = 16384;

// The Python wrapper's letterbox (Models/inference/auto_speed_infer.py:15-43; vp_detect_preprocess_pil): Pillow's BILINEAR resize is
// launch_pil_resample (mean 0, std 1, norm_form 0: its planes are u8 / 255, one IEEE division) into `src`; this kernel pastes those planes into the
// canvas of 114 / 255.
struct LetterboxPasteParams {
  const float* src;      // [3][new_h][new_w] planes R, G, B of the resized image
  int new_w, new_h, pad_x, pad_y;
  int out_h, out_w;
  float* out;            // [3][out_h][out_w]
};

struct FcParams {
  const float* x;
  const float* w;  // [N][K]
  // VP_WEIGHTS_FP8, real storage (round 4): when non-null the matrix is OCP e4m3 CODES [N][K] (one byte per weight; w is null) and
  // wscale8[n] the row's quantisation scale: out[n] = act(b[n] + wscale8[n] * sum_k q[n][k] x[k])
  const uint8_t* w8;
  const float* wscale8;
  const float* b;
  float* out;
  int N, K, act;
  // per-row activations of a small stacked matrix (N <= 4): byte n = ActFn of row n; 0 = `act` for every row (AutoDrive's three scalar heads in one launch)
  unsigned act_rows;
  int rows_kernel;       // 1: a thread per row (fc_rows_kernel: K <= 64, N >= 2048 -- fc_rows_ok); 0: two rows per wave
  const float* partial;  // optional: x = mean over nslab partial sums (avg-pool input, scene_context.py:27)
  int nslab, Kstride;
  float inv_hw;
};

bool fc_rows_ok(const FcParams& p);

struct CtxConv1Params {
  const float* map;  // [H][W] fp32
  int H, W;
  const float* w;    // [9][C]
  const float* b;    // [C]
  ActView out;
  int act;           // ACT_GELU (scene_context.py:46-47) or ACT_SILU (CTX.ctx0, common_layers.py:216-217)
  int scaled;        // VP_ACT_SCALE: != 0 -> the result is stored times out_mul (2^-s_out); 0: out_mul is not read
  float out_mul;
};

// Round 5: the matvec that BUILDS the one-channel map and the 3x3 convolution that reads it, in one launch (ctx_exp_conv1_kernel):
//   scene networks: context_layer_2 (Linear 800 -> 200 + sigmoid, reshaped 10x20: scene_context.py:36-43) + context_layer_3 (conv 1 -> 128 + GELU, :46-47);
//   AutoDrive CTX : exp0 (C -> H*W, SiLU twice: common_layers.py:210-213) + ctx0 (conv 1 -> C/2 + SiLU, :216-217).
// fc.out is unused (the map never leaves LDS); fc.partial / nslab as for launch_fc; cv.map is unused.
struct CtxExpConv1Params {
  FcParams fc;
  CtxConv1Params cv;
  int tile;     // square pixel patch per workgroup: 16, 8 or 2 -- the (tile + 2)^2 map rows under it should fit ONE pass of 256 / glanes rows
  int glanes;   // lanes that share one row of the matvec (a power of two <= 64): few enough that a lane's pieces of a row are <= ~16 loads
};
bool ctx_exp_conv1_ok(const CtxExpConv1Params& p);
hipError_t launch_ctx_exp_conv1(const CtxExpConv1Params& p, hipStream_t st);

struct FusionParams {
  ActView f[5];
  int creal[5];   // 32,24,40,80,1280
  int shift[5];   // 4,3,2,1,0
  ActView out;    // 10x20 x 1472 (1456 real)
  int Creal_out;
  int octets;     // 1: one workgroup per output pixel, 16-byte pieces, window slices meeting in LDS (fusion_octets_ok); 0: a thread per output element
};
bool fusion_octets_ok(const FusionParams& p);

// tile ids: 0 = 128co x 128px, 1 = 64co x 128px, 2 = 64co x 64px, 3 = 32co x 128px ; bk = 32 | 64
hipError_t launch_conv_gemm(const ConvGemmParams& p, int tile, int bk, bool split, hipStream_t st);
int conv_tile_co(int tile);
int conv_tile_px(int tile);
// 3x3 halo kernel (kernels_conv3x3.hip); weights packed [cin/32][9][CoutW][32].
// halo tile ids: 0 = 128co x 16x16 px, 1 = 128co x 8x16, 2 = 64co x 16x16, 3 = 64co x 8x16, 4 = 32co x 8x16
hipError_t launch_conv3x3_halo(const ConvGemmParams& p, int tile, bool split, hipStream_t st);
// halo tiles 6 - 8: the pipelined fp16x3 kernels (kernels_conv3x3_x3.hip); conv + bias + {GELU, none}, NHWC
bool conv3x3_x3_supported(const ConvGemmParams& p, int shape);
hipError_t launch_conv3x3_x3(const ConvGemmParams& p, int shape, hipStream_t st);
int halo_tile_co(int tile);
int halo_tile_px(int tile);
int halo_tile_th(int tile);
// halo tile 13, VP_MFMA_FP8 (kernels_conv3x3.hip conv3x3_f8_kernel): e4m3 codes in p.w8 (F8_K64 layout), row scales in p.wscale, p.f8_qmul / p.f8_smul =
// 2^-qexp / 2^qexp; conv + bias + {GELU, none}, one fp16 plane in and out, NHWC, Cin and CoutW multiples of 64, no split-K
bool conv3x3_f8_supported(const ConvGemmParams& p);
hipError_t launch_conv3x3_f8(const ConvGemmParams& p, hipStream_t st);
// out[i] = e4m3_quantize(in[i], mul) (common.hpp): the kernel's quantiser over an array
hipError_t launch_fp8_quantize(const half_t* in, size_t n, float mul, uint8_t* out, hipStream_t st);

// small-map 3x3 of the parity mode (kernels_conv3x3_map.hip; halo tile id 11): a workgroup = 32 output channels x a K slice x all 800 pixels of a
// 20x40 region; weights packed by conv3x3_map_pack_index; always finishes through splitk_finish_kernel (p.partial required, nsplit >= 1)
int conv3x3_map_geometry(int H, int W);  // 1 = 20x40 regions (neck), 2 = 10x20 regions (context block), 0 = neither
bool conv3x3_map_shape_ok(int H, int W, int cin_pad, int coutw);
size_t conv3x3_map_pack_index(int co, int ci, int t, int cin_pad);
size_t conv3x3_map_pack_index_k32(int co, int ci, int t, int cin_pad);   // fp16 engines: steps of 32 channels, plane = (ci >> 4) & 1
bool conv3x3_map_supported(const ConvGemmParams& p);
hipError_t launch_conv3x3_map(const ConvGemmParams& p, hipStream_t st);
// halo tile 12 ("map2", round 5): the map kernel on 64-channel weight slabs (two M tiles per wave), parity mode, 20x40 regions; weights packed by
// conv3x3_map2_pack_index; always finishes through splitk_finish_kernel
bool conv3x3_map2_shape_ok(int H, int W, int cin_pad, int coutw);
bool conv3x3_map2_supported(const ConvGemmParams& p);
size_t conv3x3_map2_pack_index(int co, int ci, int t, int cin_pad);
hipError_t launch_conv3x3_map2(const ConvGemmParams& p, hipStream_t st);
// last convolution of a head: 3x3, 64 / 128 channels -> <= 4 logit channels, fp32 NCHW + fused decode (kernels_head.hip); weights packed
// as for halo tile 4; zeros = the engine's zero page (>= 16 bytes of zeros in device memory)
bool head_conv_supported(const ConvGemmParams& p);
hipError_t launch_head_conv(const ConvGemmParams& p, const void* zeros, hipStream_t st);
// ConvTranspose (+ skip link) GEMM on the small maps: 8 waves, both operands by LDS-DMA three K steps deep (kernels_gemm_dma.hip)
bool gemm_dma_shape_ok(int M, int ncols, int cin_pad, int cin2_pad, int cstore);
size_t gemm_dma_pack_index(int n, int k, int kw);  // host packing of its weights (LDS image order per 256 x 32 tile)
bool gemm_dma_supported(const ConvGemmParams& p, bool split);
hipError_t launch_gemm_dma(const ConvGemmParams& p, hipStream_t st);
// register-stationary weights, pixel tiles by LDS-DMA (kernels_convt_rs.hip): K = 128, or 256 + 32 with the skip link; both precisions
bool convt_rs_supported(const ConvGemmParams& p, bool split);
int convt_rs_shape_case(int H, int W, int cin_pad, int cin2_pad, int ncols, int cstore);  // 0 = not covered
hipError_t launch_convt_rs(const ConvGemmParams& p, hipStream_t st);
// ---- composed up-sampling stage (kernels_upconv.hip, round 6) ------------------------------------------------------------------------
// ConvTranspose2d(k2, s2) [+ Conv1x1(skip)] followed by Conv3x3 with NO nonlinearity in between (scene_neck.py:29-35,41-46,52-57;
// scene_seg_head.py:24-29,35-38; scene_3d_head.py:26-31,38-41) is ONE linear map: a transposed convolution with a 4x4 kernel, stride 2, pad 1
// from the LOW-resolution tensor -- per output phase (Y & 1, X & 1) a 2x2 convolution of it -- plus a 3x3 convolution of the skip tensor with
// pre-multiplied weights, plus a bias that depends only on which of the 9 high-resolution taps are inside the map.  The weights are composed
// at load (upconv_compose: fp64 accumulation on the device) and the stage is ONE launch: 0.40-0.51x the matrix work of the two it replaces.
struct UpconvParams {
  const half_t* in_hi;   // low-resolution input  H x W x Cin (NHWC, Cin a multiple of 32), (hi, lo)
  const half_t* in_lo;
  const half_t* sk_hi;   // skip tensor 2H x 2W x Cs (Cs a multiple of 32) or null (Cs = 0)
  const half_t* sk_lo;
  int H, W, Cin, Cs;
  const half_t* w_hi;    // [4 phases][S steps][CoutW][32] in LDS image order (upconv_pack_index), S = upconv_steps(Cin, Cs)
  const half_t* w_lo;
  const float* bias;     // [9][CoutW]: (row class * 3 + column class), class 0 = first row / column of the OUTPUT map, 2 = last, 1 = inside
  const float* wscale;   // [4][CoutW] 2^-prescale of the weight rows of each phase (ConvGemmParams::wscale)
  int CoutW, Ncols, Cstore;
  half_t* out_hi;        // 2H x 2W x Cstore
  half_t* out_lo;
  int act;               // ACT_GELU | ACT_NONE
  int nsplit;            // K slices over the chunk list (> 1: fp32 partials + upconv_finish_kernel)
  float* partial;        // [nsplit][4 H W][CoutW]
  int compact;           // 1: the compacted form (runs of row-major pixels instead of patches, kernels_upconv.hip); needs upconv_compact_fits
};
// shapes: 6 = 8 waves, 16x16 low-resolution pixels x 128 channels per phase (one workgroup per CU); 7 = 4 waves, 8x16 pixels x 128 channels (two per CU)
bool upconv_supported(const UpconvParams& p, int shape);
// whether the compacted form's halo windows of an H x W map fit the shape's LDS plan (maps up to 48 columns wide on shape 7, ~60 on shape 6)
bool upconv_compact_fits(int H, int W, int shape);
// The K axis of one output phase (py, px) is a list of 32-channel CHUNKS, each with its own tap list (a K "step" = one chunk x one tap = one weight
// tile of CoutW x 32 and one shifted read of the chunk's halo image):
//   chunks [0, Cin / 32): the low-resolution input, 4 taps (a, b) in {0, 1}^2 = low-resolution pixel (y + py - 1 + a, x + px - 1 + b);
//   then per CLASS (qy, qx) of skip pixels (the skip tensor seen as four half-resolution images S[qy][qx](y, x) = skip(2y + qy, 2x + qx)), Cs / 32
//   chunks each: the taps of the 3x3 window around output pixel (2y + py, 2x + px) that fall on that class -- 2 per axis where the class bit differs
//   from the phase bit (high-resolution taps 0 and 2: a = 0, 1), 1 where it is equal (tap 1: a = 1 - py).  Class order (1-py, 1-px) [4 taps],
//   (1-py, px) [2], (py, 1-px) [2], (py, px) [1]: 9 * Cs / 32 steps, neighbours in the order share their cache lines.
// tap k of a chunk: a = a0 + k / nb, b = b0 + k % nb; the halo image (origin = low-resolution pixel (y0 - 1, x0 - 1) of the workgroup's patch) is read
// at rows + py + a, columns + px + b.
struct UpconvChunk {
  int skip, ch0, qy, qx, nt, nb, a0, b0, step0;
};
__host__ __device__ inline UpconvChunk upconv_chunk(int c, int py, int px, int cin_pad, int cs_pad) {
  const int kcx = cin_pad >> 5, kcs = cs_pad >> 5;
  UpconvChunk d;
  if (c < kcx || kcs == 0) {
    d.skip = 0; d.ch0 = c << 5; d.qy = 0; d.qx = 0; d.nt = 4; d.nb = 2; d.a0 = 0; d.b0 = 0; d.step0 = 4 * c;
    return d;
  }
  const int r = c - kcx, cls = r / kcs, cc = r - cls * kcs;
  d.skip = 1;
  d.ch0 = cc << 5;
  d.qy = cls < 2 ? 1 - py : py;
  d.qx = (cls & 1) ? px : 1 - px;
  const int na = d.qy != py ? 2 : 1;
  d.nb = d.qx != px ? 2 : 1;
  d.a0 = na == 2 ? 0 : 1 - py;
  d.b0 = d.nb == 2 ? 0 : 1 - px;
  d.nt = na * d.nb;
  const int cls_step0 = cls == 0 ? 0 : (cls == 1 ? 4 : (cls == 2 ? 6 : 8));
  d.step0 = 4 * kcx + cls_step0 * kcs + cc * d.nt;
  return d;
}
__host__ __device__ inline int upconv_chunks(int cin_pad, int cs_pad) { return (cin_pad >> 5) + 4 * (cs_pad >> 5); }
__host__ __device__ inline int upconv_steps(int cin_pad, int cs_pad) { return 4 * (cin_pad >> 5) + 9 * (cs_pad >> 5); }   // K steps of one phase
// packed position of weight element (phase, step, output channel co, channel i of the step's 32): [phase][step][CoutW][32] with the 16-byte pieces of
// a row XOR-swizzled by (co >> 2) & 3 -- the LDS image of a (CoutW x 32) tile, so the LDS-DMA copy is linear (as halo tiles 6 - 9, engine_dispatch.cpp)
inline size_t upconv_pack_index(int phase, int step, int co, int i, int steps, int coutw) {
  const int i_sw = ((((i & 31) >> 3) ^ ((co >> 2) & 3)) << 3) | (i & 7);
  return (((size_t)phase * steps + step) * coutw + co) * 32 + i_sw;
}
hipError_t launch_upconv(const UpconvParams& p, int shape, hipStream_t st);
// fp64-accumulating GEMM of the weight composition: C[g][m][n] = sum over the group's (A_i, B_i) pairs of sum_k A_i[m][k] * B_i[n][k] (fp32 in, fp64 out)
struct ComposeGemmParams {
  const float* a[4];   // [M][K]
  const float* b[4];   // [N][K]
  int pairs, M, N, K;
  double* c;           // [M][N]
};
hipError_t launch_compose_gemm(const ComposeGemmParams* groups_dev, int n_groups, int M, int N, hipStream_t st);
hipError_t launch_preprocess(const PreprocessParams& p, hipStream_t st);
hipError_t launch_pil_resample(const PilResampleParams& p, hipStream_t st);  // both passes
hipError_t launch_stem(const StemParams& p, hipStream_t st);
hipError_t launch_dwconv(const DwParams& p, hipStream_t st);
bool mbconv_front_supported(const MbFrontParams& p);
hipError_t launch_mbconv_front(const MbFrontParams& p, hipStream_t st);
hipError_t launch_letterbox(const LetterboxParams& p, hipStream_t st);
hipError_t launch_detect_nms(const DetectParams& p, DetectRule rule, hipStream_t st);
inline hipError_t launch_detect_decode_nms(const DetectParams& p, hipStream_t st) { return launch_detect_nms(p, kDetectPerClass, st); }  // the earlier name: callers built against it keep compiling
hipError_t launch_letterbox_paste(const LetterboxPasteParams& p, hipStream_t st);
bool mbconv_back_supported(const MbBackParams& p);
hipError_t launch_mbconv_back(const MbBackParams& p, hipStream_t st);
hipError_t launch_pool_partial(const PoolParams& p, hipStream_t st);
hipError_t launch_zero_u64(unsigned long long* p, size_t n, hipStream_t st);
// The fused average pool spreads its atomics over `replicas` rows: same-address atomics serialise in L2 (measured:
// 100+ per address cost 30 us on the 80x160 layers), so layers with many workgroups get up to 64 rows.
constexpr int kSeMaxReplicas = 64;
// squeeze-excite tail of an MBConv block in one launch: means, squeeze FC, excite FC, gate folded into the projection weights
hipError_t launch_se_gate_scale(const SeParams& se, const ScaleWParams& sw, hipStream_t st);
hipError_t launch_fc(const FcParams& p, hipStream_t st);
hipError_t launch_ctx_conv1(const CtxConv1Params& p, hipStream_t st);
hipError_t launch_fusion(const FusionParams& p, hipStream_t st);
hipError_t launch_decode_mask(const float* logits, int C, int HW, int mode, uint8_t* out, hipStream_t st);
hipError_t launch_resize_nearest(const uint8_t* src, int sw, const int* ytab, const int* xtab, int oh, int ow, uint8_t* dst,
                                 hipStream_t st);
hipError_t launch_resize_bilinear_f32(const float* src, int sw, const int* yi, const float* yf, const int* xi, const float* xf,
                                      int oh, int ow, float* dst, hipStream_t st);
hipError_t launch_minmax_f32(const float* src, size_t n, unsigned* mm, hipStream_t st);
constexpr int VP_PROBE_BLOCKS = 64;  // words of the range probe's verdict
hipError_t launch_finite_probe(const float* src, size_t n, unsigned* flags, hipStream_t st);  // flags[0..VP_PROBE_BLOCKS) = per-workgroup 0 / 1, overwritten every pass
hipError_t launch_depth_colorize(const float* src, size_t n, const unsigned* mm, const uint8_t* lut, uint8_t* dst, hipStream_t st);
hipError_t launch_viz_blend(const uint8_t* mask, int mw, const int* ytab, const int* xtab, const uint8_t* frame, int stride, int oh, int ow,
                            const uint8_t* lut, int frame_is_rgb, uint8_t* dst, hipStream_t st);
hipError_t launch_nchw_to_act(const float* src, int Creal, const ActView& a, hipStream_t st);
hipError_t launch_act_to_nchw(const ActView& a, int Creal, float* dst, hipStream_t st, float mul = 1.0f);  // dst = (hi + lo) * mul (VP_ACT_SCALE: 2^s of the tensor)
// VP_ACT_SCALE calibration (kernels_misc.hip act_absmax_kernel): result[0] = bit pattern of max |hi + lo| (fp32, non-finite elements left out) over the
// c real channels of an h x w tensor with channel pitch c_pitch (c_pitch and the plane pointers multiples of 8 elements), result[1] = count of
// non-finite elements.  Integer max / add only: the same bits whatever order the workgroups finish in.  The caller zeroes result[0..2) first.
hipError_t launch_act_absmax(const half_t* hi, const half_t* lo, int c, int h, int w, int c_pitch, unsigned* result, hipStream_t st);
// Range survey (kernels_misc.hip act_exp_hist_kernel), arguments as launch_act_absmax: result[k] += elements with floor(log2 |hi + lo|) == VP_HIST_EXP_MIN + k
// (k < VP_HIST_BINS), result[VP_HIST_BINS] += exact zeros, result[VP_HIST_BINS + 1] += real elements visited; non-finite elements in neither a bin nor the
// zeros.  Integer adds only.  The caller zeroes the VP_HIST_WORDS words first.
constexpr int VP_HIST_BINS = 40, VP_HIST_EXP_MIN = -24, VP_HIST_WORDS = VP_HIST_BINS + 2;   // == VP_RANGE_BINS / VP_RANGE_EXP_MIN of vp_hip.h (vp_api.cpp checks)
hipError_t launch_act_exp_hist(const half_t* hi, const half_t* lo, int c, int h, int w, int c_pitch, unsigned long long* result, hipStream_t st);

// ---- AutoDrive blocks (kernels_autodrive.hip)
// channel-slice copy: dst[pix][dst_off + c] = src[pix][src_off + c], c < nch (torch.cat / split / chunk along C)
hipError_t launch_chan_copy(const ActView& src, int src_off, const ActView& dst, int dst_off, int nch, hipStream_t st);
// MaxPool2d(5, stride 1, pad 2) on a channel slice (SPPF, common_layers.py:236-243)
hipError_t launch_maxpool5(const ActView& src, int src_off, const ActView& dst, int dst_off, int nch, hipStream_t st);
// SPPF's pyramid in one launch: dst slice 0 = src[0, nch), slices 1..3 = the 5x5 / 9x9 / 13x13 clipped window maxima (= three chained MaxPool2d(5, 1, 2))
bool sppf_pool_ok(const ActView& src, const ActView& dst, int nch);   // maps of at most 512 pixels (one workgroup holds an octet's map)
hipError_t launch_sppf_pool(const ActView& src, const ActView& dst, int nch, hipStream_t st);
struct AttnParams {
  ActView qkv;   // [HW][heads * (2*dk + dv)]: per head q(dk) | k(dk) | v(dv)   (Attention.forward, common_layers.py:95-99)
  ActView out;   // [HW][heads * dv] = v @ softmax(q^T k * scale)^T
  ActView vout;  // [HW][heads * dv] copy of v (input of the depthwise positional conv); same row pitch C as out, or the launch is refused
  int heads, dk, dv;
  float scale;
  int qblock;    // 4: four query tokens per workgroup (attention_block_kernel: dk = 32, dv = 64, <= 1760 tokens); 0: one workgroup per query token
  // VP_ACT_SCALE: qkv, out and vout carry ONE exponent s (tied at plan time): v -> vout is a copy and out a convex combination of v rows, so both are
  // homogeneous in v; the logits need true q . k, which the engine folds into `scale` (scale * 2^(2 s), exact) when it launches -- no device change
};
bool attention_block_ok(const AttnParams& p);
hipError_t launch_attention(const AttnParams& p, hipStream_t st);
struct DwPlainParams {
  ActView in, out;   // out = [add +] act(dwconv3x3(in)) (BN folded); Attention's positional conv (common_layers.py:103): no activation, add given
  ActView add;       // add.hi == nullptr: no add (the detector head's class branch, auto_speed_head.py:45,47)
  const float* w;    // [9][C]
  const float* b;    // [C]
  int act;           // ActFn applied before the add; 0 (ACT_NONE) = identity
  // VP_ACT_SCALE: scaled != 0 -> in is read times in_mul (2^s_in), add times add_mul (2^s_add), the result stored times out_mul (2^-s_out); 0: not read
  int scaled;
  float in_mul, add_mul, out_mul;
};
hipError_t launch_dwconv_plain(const DwPlainParams& p, hipStream_t st);

// ---- AutoSpeed detector network (neck: kernels_autodrive.hip; head decode: kernels_detect.hip)
// out[:, 0 : a_nch] = nearest x2 of a[:, a_off : a_off + a_nch], out[:, a_nch : a_nch + b_nch] = b[:, b_off : b_off + b_nch]  (auto_speed_neck.py:20-22)
struct Upsample2CatParams {
  ActView a, b, out;   // a: H x W (C = row pitch), b and out: 2H x 2W
  int a_off, a_nch, b_off, b_nch;   // multiples of 8
};
bool upsample2_cat_ok(const Upsample2CatParams& p);
hipError_t launch_upsample2_cat(const Upsample2CatParams& p, hipStream_t st);
// AutoSpeedHead.forward in eval mode behind the last convolutions (auto_speed_head.py:57-66) + DFL (common_layers.py:143-146), all levels in one launch
struct DetectHeadLevel {
  ActView box;   // [H][W][>= 64]: 4 sides x 16 bins, channel = side * 16 + bin
  ActView cls;   // [H][W][>= nc] class logits
  int first;     // index of the level's first anchor in the output rows
  float stride;
  // VP_ACT_SCALE: DetectHeadParams::scaled != 0 -> box is read times box_mul (2^s_box), cls times cls_mul (2^s_cls): the softmax, the sigmoid and the box
  // arithmetic see true values, the fp32 output is true-valued; 0: not read
  float box_mul, cls_mul;
};
struct DetectHeadParams {
  DetectHeadLevel lv[3];
  int nc, total;   // classes; anchors over all levels (10752 at 512 x 1024)
  float* out;      // fp32 [4 + nc][total]: cx, cy, w, h in input pixels, then sigmoid class scores
  int scaled;      // VP_ACT_SCALE: != 0 -> the levels' box_mul / cls_mul apply
};
hipError_t launch_detect_head_decode(const DetectHeadParams& p, hipStream_t st);

// ---- AutoSteer lane-perception head (auto_steer_percept_head.py:45-68; rowpair_conv: kernels_autodrive.hip, lane_rows_head: kernels_detect.hip)
// Conv2d(cin -> 32, kernel (2,1), stride (2,1), bias) + SiLU: out(y, x, co) = SiLU(b[co] + sum_{ky, ci} w[ky * cin + ci][co] * in(2y + ky, x, ci)), fp32 FMAs
// in that k order.  `out` may be an alias slice of a wider tensor (out.C = its row pitch).  replicate: every result is stored to the four pixels
// (2y + dy, 2x + dx) of an `out` of twice the size -- Upsample(scale_factor=2, nearest) of the result (:55).
struct RowpairConvParams {
  ActView in;        // H x W x >= cin (an odd last row is ignored, as Conv2d does)
  int cin;           // multiple of 8, <= 64
  const float* w;    // [2 * cin][32]
  const float* b;    // [32]
  ActView out;       // (H / 2) x W, or H x 2W with replicate; 32 channels are stored at out.hi / out.lo
  int replicate;
  // VP_ACT_SCALE: scaled != 0 -> in is read times in_mul (2^s_in), the result stored times out_mul (2^-s_out) behind SiLU (plain and replicated store); 0: not read
  int scaled;
  float in_mul, out_mul;
};
bool rowpair_conv_ok(const RowpairConvParams& p);
hipError_t launch_rowpair_conv(const RowpairConvParams& p, hipStream_t st);
// Everything behind `features` (:58-85), one workgroup per row, one thread per column (W = 256): c1 and c2 as ONE 2-output 3x3 convolution (BN folded,
// taps outside the map skipped); lanes: SiLU, SiLU, softmax over the row, expectation of the column index / W; height: SiLU, SiLU, h1 over 16 groups of
// 16 columns + SiLU, h2 over the 16 results + SiLU.
struct LaneRowsHeadParams {
  ActView features;  // H x 256 x cin
  int cin;           // multiple of 8, <= 64
  const float* w;    // [9 taps (ky * 3 + kx)][cin][2 outputs (c1, c2)]
  const float* hw;   // [16] h1 weights, [16] h2 weights, then the biases of c1, c2, h1, h2
  float* out;        // fp32 [2][H]: xp, h_vector
  // VP_ACT_SCALE: scaled != 0 -> features is read times in_mul (2^s_features); xp / h_vector are true-valued either way; 0: not read
  int scaled;
  float in_mul;
};
bool lane_rows_head_ok(const LaneRowsHeadParams& p);
hipError_t launch_lane_rows_head(const LaneRowsHeadParams& p, hipStream_t st);

// ---- vp_metric (include/vp_hip.h; kernels_misc.hip metric_*): the validation scores of the segmentation and depth trainers, one record per frame.
// No kernel talks to another workgroup of its own launch: a workgroup writes its partial, and the NEXT launch folds the partials in index order (every
// workgroup of it repeats the same fold), so a record has the same bits on every run.  Integer atomics only (LDS histograms, the ten u32 counters).
// MetricRecord is vp_metric_frame's layout (vp_api.cpp checks it).
struct MetricRecord {
  int kind;
  unsigned I[3], P[3], G[3];
  unsigned nonfinite, n, kept;
  float q_lo, q_hi, q, mae, mel;
};
constexpr int kMetricBlocks = 128;   // workgroups (of 256) of every partial-writing launch, at most
constexpr unsigned kMetricMaxN = 1u << 24;
// metric_seg_count_kernel: logits fp32 [c][n] (c 1 or 3); the ground truth is gt (u8 [n], gt_form 0: class index, 1: bit c = plane c) or, with gt null,
// the class ref's logits [c][n] predict.  Adds into rec->I / P / G / nonfinite (zeroed by the caller) and stores rec->kind and rec->n.
struct MetricSegParams {
  const float* logits;
  const float* ref;
  const uint8_t* gt;
  int c, gt_form, kind;
  unsigned n;
  MetricRecord* rec;
};
hipError_t launch_metric_seg_count(const MetricSegParams& p, hipStream_t st);
// the depth chain's scratch, owned by the caller: D and the bits of |D| ([n] each), the three pooled scales of D one after the other ([n / 4 + n / 16 + n / 64]
// at most), and the partials
struct MetricStatPartial {
  double sum[2];
  float mn[2], mx[2];
  unsigned bad[2];
};
struct MetricKeptPartial {
  double sum;
  unsigned long long count;
};
struct MetricDepthParams {
  const float* pred;   // [h][w]
  const float* gt;     // [h][w]
  int h, w, kind;
  float* d;            // [n]
  unsigned* a_bits;    // [n]
  float* pooled;       // scales 1 .. 3
  MetricStatPartial* stat;   // [kMetricBlocks]
  MetricKeptPartial* kept;   // [kMetricBlocks]
  double* edge;              // [4][kMetricBlocks]
  unsigned* sel;             // [2]: the bits of the order statistics lo and lo + 1
  unsigned* sel_scratch;     // metric_select_scratch_bytes(h * w)
  MetricRecord* rec;
};
size_t metric_pooled_elems(int h, int w);
// the whole chain for one frame: stats, D and |D|, select, kept count and sum, the four edge sums, the record.  h, w >= 8, h * w <= kMetricMaxN.
hipError_t launch_metric_depth(const MetricDepthParams& p, hipStream_t st);
// ranks k0 and k1 of n u32 keys in ascending order: out[0], out[1].  Four 8-bit passes of per-workgroup LDS histograms, each folded by the launch behind it.
size_t metric_select_scratch_bytes(unsigned n);
hipError_t launch_metric_select(const unsigned* bits, unsigned n, unsigned k0, unsigned k1, unsigned* scratch, unsigned* out, hipStream_t st);
// the rank pair of the 0.9 quantile with linear interpolation over n values and its weight: lo = floor(r), w = r - lo with r = fp32(0.9f * (n - 1))
inline void metric_quantile_rank(unsigned n, unsigned* lo, unsigned* hi, float* w) {
  const float r = 0.9f * (float)(n - 1);
  const float f = (float)(unsigned)r;
  *lo = (unsigned)r;
  *hi = *lo + 1 < n ? *lo + 1 : n - 1;
  *w = r - f;
}

// ---- vp_metric, lane part (include/vp_hip.h "vp_metric: the lane networks"; kernels_misc.hip metric_lanes_* / metric_rows_*): the EgoLanes trainer's loss
// as a validation score (ego_lanes_trainer.py:280-356) and the per-line stage of the AutoSteer trainer's val() (auto_steer_trainer.py:203-222).
// Lanes: per plane c the sum of the per-pixel BCE-with-logits terms, and five edge sums: scale 0 on D0 = relu(x) - g, scales 1 .. 4 on the 2x2 mean pools of
// E = Threshold(0, 1)(relu(x)) - g.  Two shapes of the same device code:
//   small    h * w <= kMetricLanesLdsN: ONE launch of three workgroups, plane c in workgroup c, D0 and the four pooled levels in LDS;
//   general  prep (grid nb x 3: BCE partials, D0 and pooled level 1 into scratch), then one edge launch per scale (grid nb_s x 3; it pools into the next level).
// Both write partials (double, one per workgroup) that metric_lanes_finish_kernel (one workgroup) folds in index order through the fixed tree.
// LanesRecord is vp_metric_lanes_frame's layout, RowsRecord vp_metric_rows_line's (vp_api.cpp checks both).
struct LanesRecord {
  float bce[3], edge[3][5], loss[3], score;
  unsigned n, nonfinite;
};
constexpr unsigned kMetricLanesLdsN = 12800;       // the production 80 x 160 plane
constexpr unsigned kMetricLanesMaxN = 1u << 22;
constexpr int kMetricLanesMinSide = 16;            // four 2x2 pools leave a pixel
// ground truth of a lanes record: fp32 planes [3][h][w]; u8 [h][w], bit c = plane c; u8 [4h][4w], bit c of the OR over each 4x4 block; the planes
// ref's logits [3][h][w] predict (1 where > 0)
enum { kLanesGtPlanes = 0, kLanesGtBits = 1, kLanesGtBits4x = 2, kLanesGtRef = 3 };
struct MetricLanesParams {
  const float* logits;   // [3][h][w]
  const void* gt;
  int gt_form, h, w;
  float* d0;             // general path: [3][n]
  float* pooled;         // general path: [3][metric_lanes_pooled_elems(h, w)], the four levels of a plane one after the other
  double* part;          // [3][7][kMetricBlocks]: BCE sum, five edge sums, non-finite count
  LanesRecord* rec;
};
size_t metric_lanes_pooled_elems(int h, int w);
hipError_t launch_metric_lanes(const MetricLanesParams& p, hipStream_t st);
// Rows: one workgroup per line.  Term r = |xp[r] * m - txp[r] * mt| with m = h[r] > 0.5, mt = th[r] > 0.5 as fp32 operations; the sums of the terms and of h
// are formed in double: element r into slot r mod 256 in ascending r, the 256 slots by the fixed tree; dist / conf = fp32(sum / rows).
struct RowsRecord {
  float dist, conf;
  unsigned tp, valid, target_valid;
};
constexpr int kMetricRowsMaxLines = 8, kMetricRowsMaxRows = 1024, kMetricRowsMaxThr = 8;
struct MetricRowsParams {
  const float *xp, *hv, *txp, *thv;   // [n_lines][rows] each
  int n_lines, rows, n_thr;
  double thr[kMetricRowsMaxThr];
  RowsRecord* rec;                    // [n_lines]
};
hipError_t launch_metric_rows(const MetricRowsParams& p, hipStream_t st);

// ---- vp_metric, label part (include/vp_hip.h "vp_metric: ground truth from label files"; kernels_misc.hip label_*): a dataset's label file, as decoded,
// becomes the ground truth of the network's output size on the device (load_data_scene_seg.py:55-166, load_data_scene_3d.py:59-66, the nearest resize
// of augmentations.py:133-177).  Colour / mask labels: label_stats_kernel counts the full-resolution crop (the part of it inside the image; the launcher
// knows the rest in closed form) into one integer partial per workgroup, label_gt_kernel samples through the two nearest tables, classifies and stores,
// and its workgroup 0 folds the partials into the record.  Depth labels: label_minmax_kernel writes one partial per workgroup, every workgroup of
// label_depth_gt_kernel folds them in index order before it normalises.  Integer folds and a fixed tree: records are bit-identical run to run.
// LabelRecord is vp_label_frame's layout (vp_api.cpp checks it).
struct LabelRecord {
  int kind;   // 0 colour label, 2 mask label, 1 depth label: the engine kind the ground truth is for
  unsigned n, freq[3], unmatched, outside, nonfinite;
  double mn, mx;
};
constexpr int kLabelMaxColours = 16, kLabelMaxSide = 16384;
constexpr int kLabelCropMin = -16384, kLabelCropMax = 32768;   // every box coordinate: cw * ch stays below 2^32
enum { kLabelF32 = 0, kLabelF64 = 1 };
struct LabelSegParams {
  const uint8_t* label;   // [h][stride bytes], channels bytes per pixel (3: R, G, B)
  int channels, h, w, stride;
  int l, t, cw, ch;       // the crop box: pixel (y, x) of the crop is image pixel (t + y, l + x), (0, 0, 0) / 0 outside the image
  int n_colours;          // channels 3: table rows, the first equal row gives the class
  unsigned rgb[kLabelMaxColours];   // r | g << 8 | b << 16
  unsigned char cls[kLabelMaxColours];
  const int* ty;          // [oh] nearest table ch -> oh
  const int* tx;          // [ow] nearest table cw -> ow
  int oh, ow;
  uint8_t* gt;            // [oh][ow]: the class or 255 (channels 3), the sampled byte (channels 1)
  unsigned* part;         // [kMetricBlocks][4]: freq[3], unmatched
  LabelRecord* rec;
};
hipError_t launch_label_seg(const LabelSegParams& p, hipStream_t st);
struct LabelExtPartial {
  double mn, mx;
  unsigned bad, nan;   // non-finite values; NaNs among them
};
struct LabelDepthParams {
  const void* label;      // [h][stride elements] fp32 or fp64
  int dtype, h, w, stride;
  const int* ty;          // [oh] nearest table h -> oh
  const int* tx;          // [ow] nearest table w -> ow
  int oh, ow;
  float* gt;              // [oh][ow]
  LabelExtPartial* part;  // [kMetricBlocks]
  LabelRecord* rec;
};
hipError_t launch_label_depth(const LabelDepthParams& p, hipStream_t st);

// ---- vp_metric, detector part (include/vp_hip.h "vp_metric: the detector"; kernels_detect.hip det_val_*): the validation post-process of the detector's
// trainer (auto_speed_util.py non_max_suppression + compute_metric) on a raw tensor [4 + nc][nb].  The chain, one launch each, no workgroup talking to
// another inside a launch:
//   expand    every (box, class) pair above conf -> a 64-bit key (orderable score bits << 32 | ~candidate index) at an atomic slot; the arrival order is
//             erased by the rank (keys are unique, a rank depends on the SET of keys only)
//   rank      rank = number of greater keys, by counting: a grid of (256 keys) x (slices of 4096 keys), tiles of 1024 keys through LDS, one integer
//             atomic per key and slice
//   place     rank r < max_nms: candidate index -> order[r], class-offset corners -> boxes[r]
//   suppress  ONE workgroup: greedy in rank order, byte flags of the <= 30000 ranks in LDS, boxes in global memory, a barrier per kept box, stops at
//             max_det; writes the kept rows and {candidates, ranked, kept}
//   labels    (pair form) the kept rows of the reference chain above label_conf -> label rows
//   match     ONE workgroup: compute_metric's tp word per kept row, then the frame's record, rows and label classes behind the accumulator's running totals
constexpr int kDetValMaxNms = 30000;      // VP_DET_MAX_NMS
constexpr int kDetValMaxDet = 300;        // VP_DET_MAX_DET
constexpr int kDetValMaxClasses = 80;
constexpr int kDetValMaxBoxes = 16384;
constexpr int kDetValMaxPairs = 131072;   // nb * nc
constexpr int kDetValMaxIou = 16;
constexpr int kDetValMaxLabels = 4096;    // per frame
constexpr int kDetValRowWords = 7;        // x1, y1, x2, y2, conf, cls, tp
struct DetValParams {
  const float* raw;            // [4 + nc][nb]
  unsigned nb, nc;
  float conf, iou;
  int max_nms, max_det;
  unsigned* slots;             // [1] zeroed by launch_det_validate: the candidate count
  unsigned long long* keys;    // [nb * nc]
  unsigned* rank;              // [nb * nc]
  unsigned* order;             // [min(nb * nc, max_nms)] candidate index i * nc + c of rank r
  float* boxes;                // [min(nb * nc, max_nms)][4] class-offset corners in rank order
  float* rows;                 // out [max_det][7]: un-offset corners, score, class, tp = 0
  unsigned* counts;            // out [3]: candidates, ranked, kept
};
size_t det_val_scratch_bytes(unsigned nb, unsigned nc);
// carves slots .. boxes out of `scratch` (256-byte aligned, det_val_scratch_bytes(nb, nc))
void det_val_carve(uint8_t* scratch, DetValParams* p);
bool det_val_ok(const DetValParams& p);
hipError_t launch_det_validate(const DetValParams& p, hipStream_t st);
struct DetValLabelsParams {
  const float* rows;           // [max_det][7] of the reference chain
  const unsigned* counts;      // its [3]
  float label_conf;
  float* labels;               // out [max_det][5]: cls, x1, y1, x2, y2
  unsigned* n_labels;          // out [1]
};
hipError_t launch_det_val_labels(const DetValLabelsParams& p, hipStream_t st);
struct DetFrameRecord {        // == vp_metric_det_frame
  unsigned candidates, ranked, kept, labels, first_row;
};
struct DetRowRecord {          // == vp_metric_det_row
  float x1, y1, x2, y2, conf, cls;
  unsigned tp;
};
struct DetMatchParams {
  const float* rows;           // [max_det][7] of launch_det_validate
  const unsigned* counts;      // its [3]
  const float* labels;         // [n_labels][5]
  const unsigned* n_labels_dev;   // pair form: the count on the device (<= n_labels); else null
  int n_labels;
  int label_form;              // 0: cls, cx, cy, w, h normalised -> wh2xy, times (W, H, W, H); 1: cls, x1, y1, x2, y2 in pixels
  float W, H;
  float iou_v[kDetValMaxIou];
  int n_iou;
  unsigned* totals;            // [2] rows and labels of the accumulator so far; advanced by this launch
  DetFrameRecord* frame;       // out [1]
  DetRowRecord* rows_out;      // the accumulator's rows; this frame's go to rows_out[totals[0] ..]
  float* label_cls_out;        // the accumulator's label classes; this frame's go to label_cls_out[totals[1] ..]
};
hipError_t launch_det_val_match(const DetMatchParams& p, hipStream_t st);

// ---- vp_lanes (include/vp_hip.h; kernels_detect.hip lane_filter_kernel): the production lane filter behind an EgoLanes pass -- start points, the four
// sliding-window runs (lane x direction) and the integer moments of the collected points, one record per frame.  Geometry 80 x 160 only.
constexpr int kLaneH = 80, kLaneW = 160, kLaneRowWords = kLaneW / 32, kLaneMaxSteps = 20, kLaneRunPoints = kLaneMaxSteps * 48;
struct LaneFilterLane {
  int start_x, start_y;        // (-1, -1): no start point, everything below is empty
  int n_windows[2];            // [0] the upward run, [1] the downward run
  int n_points[2];
  int min_y, max_y;            // over the collected points; (kLaneH, -1) when there are none
  long long S[5];              // sum y^k, k = 0 .. 4
  long long T[3];              // sum x y^k, k = 0 .. 2
  short win[2][kLaneMaxSteps][4];   // per run: x, y, w, h of every window, in order
};
struct LaneFilterRecord {
  LaneFilterLane lane[2];      // ego left, ego right
};
struct LaneFilterParams {
  const float* logits;         // fp32 [3][80][160]: ego left, ego right, other lanes; 16-byte aligned
  float threshold;             // a pixel is set iff logit > threshold
  LaneFilterRecord* rec;       // out [1]
  uint16_t* points;            // out [2 lanes][2 runs][kLaneRunPoints]: x | y << 8, the first n_points[run] of each run in collection order
};
hipError_t launch_lane_filter(const LaneFilterParams& p, hipStream_t st);

}  // namespace vp

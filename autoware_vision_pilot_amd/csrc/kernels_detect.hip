// AutoSpeed detector pre / post-processing on the device (second half).  The detector network itself is a
// different model family and not part of this library; these are the two stages the reference's engines wrap around it on the CPU
// (VisionPilot/middleware_recipes/common/backends/autospeed/onnxruntime_engine.cpp; tensorrt_engine.cpp holds the same code):
//   letterbox_kernel           preprocessAutoSpeed (:71-113): resize (aspect kept) into a 114-grey canvas, / 255, planes R, G, B
//   detect_nms_kernel<false>   postProcess + applyNMS (:170-290): strict-'>' class argmax from 0, confidence threshold, xywh -> xyxy, letterbox
//                              space -> image, clamp, sort by confidence, greedy same-class IoU suppression
// and the same two stages as the Python wrapper computes them (letterbox_paste_kernel, detect_nms_kernel<true>).
// Integer / index work is bit-exact against oracle/autospeed.py; the fp32 arithmetic is the reference's, expression for expression, with
// IEEE division and without contraction (__f*_rn), so the kept set and its coordinates are bit-identical too.
#include "act_io.hpp"
#include "conv_epilogue.hpp"

namespace vp {

__global__ __launch_bounds__(256) void letterbox_kernel(const LetterboxParams p) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= p.out_w) return;
  const int rx = x - p.pad_x, ry = y - p.pad_y;
  int q[3] = {114, 114, 114};  // cv::Scalar(114, 114, 114)
  if ((unsigned)rx < (unsigned)p.new_w && (unsigned)ry < (unsigned)p.new_h) {
    const int4 xt = *reinterpret_cast<const int4*>(p.xtab + 4 * rx);
    const int4 yt = *reinterpret_cast<const int4*>(p.ytab + 4 * ry);
    const uint8_t* r0 = p.frame + (size_t)yt.x * p.stride;
    const uint8_t* r1 = p.frame + (size_t)yt.y * p.stride;
#pragma unroll
    for (int c = 0; c < 3; ++c) {  // the integer bilinear of preprocess_kernel (kernels_misc.hip)
      const int s0 = (int)r0[xt.x * 3 + c] * xt.z + (int)r0[xt.y * 3 + c] * xt.w;
      const int s1 = (int)r1[xt.x * 3 + c] * xt.z + (int)r1[xt.y * 3 + c] * xt.w;
      q[c] = min(max((((yt.z * (s0 >> 4)) >> 16) + ((yt.w * (s1 >> 4)) >> 16) + 2) >> 2, 0), 255);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)  // plane c = source byte 2 - c (BGR -> RGB); convertTo(CV_32F, 1 / 255)
    p.out[((size_t)c * p.out_h + y) * p.out_w + x] = __fmul_rn((float)q[2 - c], (float)(1.0 / 255.0));
}

hipError_t launch_letterbox(const LetterboxParams& p, hipStream_t st) {
  if (!p.frame || !p.xtab || !p.ytab || !p.out || p.new_w < 1 || p.new_h < 1 || p.pad_x < 0 || p.pad_y < 0 || p.pad_x + p.new_w > p.out_w ||
      p.pad_y + p.new_h > p.out_h)
    return hipErrorInvalidValue;
  VP_LAUNCH(letterbox_kernel, dim3((p.out_w + 255) / 256, p.out_h), dim3(256), 0, st, p);
}

// ------------------------------------------------------------------------------------------------------------- decode + NMS
// One kernel, two rules.  AGNOSTIC = false is the C++ engines' postProcess + applyNMS (onnxruntime_engine.cpp:170-290); AGNOSTIC = true is the Python
// wrapper's post_process_predictions + nms + the back-mapping of inference() (Models/inference/auto_speed_infer.py:63-83, :100-106), which
// tests/autospeed_py_ref.py restates.  One workgroup of 1024 threads: the stage is a few thousand boxes of 8 floats and inherently sequential at its
// end (greedy NMS).  The rules differ in four places (det_best_class, det_to_image in C or in E, det_iou and the class test in D, the sixth word of a
// row) and share everything else:
//   A  candidates: per box the best class and the threshold (det_best_class); survivors get a 64-bit key (score bits << 32 | ~box index) in LDS.
//      Scores are >= +0 under either rule, so their bit patterns order like the floats; ~index makes equal scores keep the box order (the
//      reference's std::sort leaves ties unspecified; torchvision's nms is stable).
//   B  bitonic sort of the keys in LDS, descending (<= 16384 keys = 128 KB).
//   C  the sorted candidates' corners cx -+ w / 2 -> scratch: mapped to the image and clamped here under the C++ rule (postProcess :198-222), left
//      in LETTERBOX pixels under the agnostic one (xywh2xyxy :45-52).
//   D  greedy suppression: a kept box i suppresses later boxes with IoU > threshold -- of its own class only (applyNMS :257-290) or whatever the
//      classes (torchvision.ops.nms) -- all threads striding over j; boxes that are already suppressed cost nothing (the flag is uniform after the
//      last barrier), so the barriers number the KEPT boxes.
//   E  compaction in order (per-thread chunks, scan in LDS).  The agnostic rule maps and clamps a kept box only now, as its row is written
//      (:101-106); its class is written as a float, the C++ rule's as the int of Detection.
constexpr int kDetThreads = 1024;

// the best class score of box i and its class.  C++ rule: strict '>' over the raw scores starting from 0 (class -1 when none is positive).  Agnostic
// rule: a sigmoid over every score (the head's scores are sigmoids already; the wrapper applies a second one, :69), the first maximum as torch.max
// finds it -- a NaN wins and stays (the box is then dropped by the threshold).
template <bool AGNOSTIC>
__device__ __forceinline__ float det_best_class(const DetectParams& p, const int i, int* cls_out) {
  const int nb = p.num_boxes;
  float best = 0.0f;
  int cls = -1, c = 4;
  if constexpr (AGNOSTIC) {
    best = sigmoid_f(p.raw[(size_t)4 * nb + i]);
    cls = 0;
    c = 5;
  }
  for (; c < p.num_attrs; ++c) {
    float s = p.raw[(size_t)c * nb + i];
    if constexpr (AGNOSTIC) s = sigmoid_f(s);
    if (s > best || (AGNOSTIC && s != s && best == best)) {
      best = s;
      cls = c - 4;
    }
  }
  *cls_out = cls;
  return best;
}

// corners in letterbox pixels -> image, (x - pad) / scale clamped to [0, orig]; the two sources nest their min and max differently
template <bool AGNOSTIC>
__device__ __forceinline__ f32x4_t det_to_image(const f32x4_t b, const DetectParams& p) {
  const auto one = [&](const float v, const int pad, const int orig) {
    const float q = __fdiv_rn(__fsub_rn(v, (float)pad), p.scale), lim = (float)orig;
    return AGNOSTIC ? fminf(fmaxf(q, 0.0f), lim) : fmaxf(0.0f, fminf(lim, q));
  };
  return f32x4_t{one(b[0], p.pad_x, p.orig_w), one(b[1], p.pad_y, p.orig_h), one(b[2], p.pad_x, p.orig_w), one(b[3], p.pad_y, p.orig_h)};
}

// computeIoU (onnxruntime_engine.cpp:239-255) / torchvision.ops.nms (no +1): the same expression; only the C++ code guards the division, so under
// the agnostic rule a 0 / 0 is NaN and suppresses nothing
template <bool AGNOSTIC>
__device__ __forceinline__ float det_iou(const f32x4_t a, const f32x4_t b) {
  const float iw = fmaxf(0.0f, __fsub_rn(fminf(a[2], b[2]), fmaxf(a[0], b[0])));
  const float ih = fmaxf(0.0f, __fsub_rn(fminf(a[3], b[3]), fmaxf(a[1], b[1])));
  const float inter = __fmul_rn(iw, ih);
  const float area_a = __fmul_rn(__fsub_rn(a[2], a[0]), __fsub_rn(a[3], a[1]));
  const float area_b = __fmul_rn(__fsub_rn(b[2], b[0]), __fsub_rn(b[3], b[1]));
  const float uni = __fsub_rn(__fadd_rn(area_a, area_b), inter);
  return AGNOSTIC || uni > 0.0f ? __fdiv_rn(inter, uni) : 0.0f;
}

__device__ __forceinline__ int det_box_of(const unsigned long long key) { return (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)); }

template <bool AGNOSTIC>
__global__ __launch_bounds__(kDetThreads) void detect_nms_kernel(const DetectParams p, const int P_max) {
  extern __shared__ __attribute__((aligned(16))) unsigned char det_smem[];
  unsigned long long* const keys = reinterpret_cast<unsigned long long*>(det_smem);      // [P_max]
  unsigned char* const flags = det_smem + (size_t)P_max * 8;                              // [P_max] 1 = suppressed
  __shared__ int n_cand;
  __shared__ int scan[kDetThreads];
  const int tid = threadIdx.x, nb = p.num_boxes;
  if (tid == 0) n_cand = 0;
  __syncthreads();
  // ---- A
  for (int i = tid; i < nb; i += kDetThreads) {
    int cls;
    const float best = det_best_class<AGNOSTIC>(p, i, &cls);
    if (AGNOSTIC ? !(best > p.conf_thresh) : best < p.conf_thresh) continue;
    const int slot = atomicAdd(&n_cand, 1);
    keys[slot] = ((unsigned long long)__float_as_uint(best) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
    p.cls[i] = cls;
  }
  __syncthreads();
  const int n = n_cand;
  int P = 1;
  while (P < n) P <<= 1;
  for (int t = n + tid; t < P; t += kDetThreads) keys[t] = 0ull;
  __syncthreads();
  // ---- B: descending bitonic sort
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < P; t += kDetThreads) {
        const int u = t ^ j;
        if (u > t) {
          const unsigned long long a = keys[t], b = keys[u];
          if (((t & k) == 0) ? a < b : a > b) {
            keys[t] = b;
            keys[u] = a;
          }
        }
      }
      __syncthreads();
    }
  // ---- C: corners of the sorted candidates
  for (int r = tid; r < n; r += kDetThreads) {
    const int i = det_box_of(keys[r]);
    const float cx = p.raw[i], cy = p.raw[(size_t)nb + i], w = p.raw[(size_t)2 * nb + i], h = p.raw[(size_t)3 * nb + i];
    const float hw = __fdiv_rn(w, 2.0f), hh = __fdiv_rn(h, 2.0f);
    f32x4_t b = {__fsub_rn(cx, hw), __fsub_rn(cy, hh), __fadd_rn(cx, hw), __fadd_rn(cy, hh)};
    if constexpr (!AGNOSTIC) b = det_to_image<false>(b, p);
    *reinterpret_cast<f32x4_t*>(p.boxes + (size_t)r * 4) = b;
    flags[r] = 0;
  }
  __threadfence_block();
  __syncthreads();
  // ---- D: greedy suppression
  for (int i = 0; i < n; ++i) {
    if (flags[i]) continue;  // uniform: nothing was written since the last barrier
    const f32x4_t bi = *reinterpret_cast<const f32x4_t*>(p.boxes + (size_t)i * 4);
    const int ci = AGNOSTIC ? 0 : p.cls[det_box_of(keys[i])];
    for (int j = i + 1 + tid; j < n; j += kDetThreads) {
      if (flags[j]) continue;
      if constexpr (!AGNOSTIC)
        if (p.cls[det_box_of(keys[j])] != ci) continue;
      if (det_iou<AGNOSTIC>(bi, *reinterpret_cast<const f32x4_t*>(p.boxes + (size_t)j * 4)) > p.iou_thresh) flags[j] = 1;
    }
    __syncthreads();
  }
  // ---- E: the kept boxes, in order
  const int per = (n + kDetThreads - 1) / kDetThreads, r0 = min(n, tid * per), r1 = min(n, r0 + per);
  int mine = 0;
  for (int r = r0; r < r1; ++r) mine += flags[r] ? 0 : 1;
  scan[tid] = mine;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int t = 0; t < kDetThreads; ++t) {
      const int v = scan[t];
      scan[t] = run;
      run += v;
    }
    p.count[0] = run;
    p.count[1] = n;
  }
  __syncthreads();
  int pos = scan[tid];
  for (int r = r0; r < r1; ++r) {
    if (flags[r]) continue;
    if (pos < p.out_cap) {
      f32x4_t b = *reinterpret_cast<const f32x4_t*>(p.boxes + (size_t)r * 4);
      if constexpr (AGNOSTIC) b = det_to_image<true>(b, p);
      const int cls = p.cls[det_box_of(keys[r])];
      Detection d;
      d.x1 = b[0];
      d.y1 = b[1];
      d.x2 = b[2];
      d.y2 = b[3];
      d.confidence = __uint_as_float((unsigned)(keys[r] >> 32));
      d.class_id = AGNOSTIC ? (int)__float_as_uint((float)cls) : cls;
      p.out[pos] = d;
    }
    ++pos;
  }
}

template <bool AGNOSTIC>
static hipError_t launch_detect_nms_rule(const DetectParams& p, const int P, hipStream_t st) {
  static LdsAttrOnce once;
  if (hipError_t e = set_max_dynamic_lds(once, reinterpret_cast<const void*>(detect_nms_kernel<AGNOSTIC>), 9 * kDetectMaxBoxes); e != hipSuccess) return e;
  hipLaunchKernelGGL(detect_nms_kernel<AGNOSTIC>, dim3(1), dim3(kDetThreads), (size_t)P * 9, st, p, P);
  return hipGetLastError();
}

hipError_t launch_detect_nms(const DetectParams& p, DetectRule rule, hipStream_t st) {
  if (!p.raw || !p.boxes || !p.cls || !p.count || (p.out_cap > 0 && !p.out) || p.num_attrs < 5 || p.num_boxes < 1 || p.num_boxes > kDetectMaxBoxes || p.out_cap < 0 ||
      !(p.scale > 0.0f))
    return hipErrorInvalidValue;
  int P = 1;
  while (P < p.num_boxes) P <<= 1;
  return rule == kDetectAgnostic ? launch_detect_nms_rule<true>(p, P, st) : launch_detect_nms_rule<false>(p, P, st);
}

// ---------------------------------------------------------------------------------------------- the Python wrapper's letterbox
// Models/inference/auto_speed_infer.py letterboxes with Pillow; tests/autospeed_py_ref.py is the restatement this kernel is held to.
// resize_letterbox + ToTensor (:24-42): Image.new("RGB", size, (114, 114, 114)), paste at (pad_x, pad_y).  The resized planes come from
// launch_pil_resample as u8 / 255 (one IEEE division: torchvision's ToTensor), so the paste is a copy; the grey is the same division of 114.
__global__ __launch_bounds__(256) void letterbox_paste_kernel(const LetterboxPasteParams p) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= p.out_w) return;
  const int rx = x - p.pad_x, ry = y - p.pad_y;
  const bool inside = (unsigned)rx < (unsigned)p.new_w && (unsigned)ry < (unsigned)p.new_h;
  const float grey = __fdiv_rn(114.0f, 255.0f);
#pragma unroll
  for (int c = 0; c < 3; ++c)
    p.out[((size_t)c * p.out_h + y) * p.out_w + x] = inside ? p.src[((size_t)c * p.new_h + ry) * p.new_w + rx] : grey;
}

hipError_t launch_letterbox_paste(const LetterboxPasteParams& p, hipStream_t st) {
  if (!p.src || !p.out || p.new_w < 1 || p.new_h < 1 || p.pad_x < 0 || p.pad_y < 0 || p.pad_x + p.new_w > p.out_w || p.pad_y + p.new_h > p.out_h)
    return hipErrorInvalidValue;
  VP_LAUNCH(letterbox_paste_kernel, dim3((p.out_w + 255) / 256, p.out_h), dim3(256), 0, st, p);
}

// ------------------------------------------------------------------------------------------------ detector head decode
// AutoSpeedHead.forward in eval mode behind the per-level convolutions (auto_speed_head.py:57-66) with DFL (common_layers.py:143-146), the three
// levels in one launch: a thread per anchor reads its 64 box channels and nc class channels as hi (+ lo) and writes one column of the fp32
// [4 + nc][total] tensor (rows are contiguous over anchors: the stores of a wave coalesce; levels concatenated P3, P4, P5, row-major inside a level).
// Arithmetic, all fp32, in this order:
//   per side s (0 = left, 1 = top, 2 = right, 3 = bottom): m = max of the 16 bins; e_i = expf(x_i - m); S = e_0 + e_1 + ... + e_15 (bin order);
//   d_s = 0 * (e_0 / S) + 1 * (e_1 / S) + ... + 15 * (e_15 / S) summed in bin order (DFL's conv weight is the constant 0..15: checked at load);
//   anchor (ax, ay) = (x + 0.5, y + 0.5);  a = (ax - d_0, ay - d_1);  b = (ax + d_2, ay + d_3);
//   cx, cy = (a + b) / 2 * stride;  w, h = (b - a) * stride;  score_c = 1 / (1 + expf(-logit_c)).
__global__ __launch_bounds__(256) void detect_head_decode_kernel(const DetectHeadParams p) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= p.total) return;
  const int li = n >= p.lv[2].first ? 2 : (n >= p.lv[1].first ? 1 : 0);
  const DetectHeadLevel& L = p.lv[li];
  const int pix = n - L.first;
  const int y = pix / L.box.W, x = pix - y * L.box.W;
  float d[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    float v[16];
    load8(L.box, (size_t)pix * L.box.C + s * 16, v);
    load8(L.box, (size_t)pix * L.box.C + s * 16 + 8, v + 8);
    if (p.scaled) {   // VP_ACT_SCALE: true logits (a power of two times the recombined hi + lo: exact)
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] *= L.box_mul;
    }
    float m = v[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) m = fmaxf(m, v[i]);
    float S = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      v[i] = expf(v[i] - m);
      S += v[i];
    }
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc += (float)i * (v[i] / S);
    d[s] = acc;
  }
  const float ax = (float)x + 0.5f, ay = (float)y + 0.5f;
  const float a0 = ax - d[0], a1 = ay - d[1], b0 = ax + d[2], b1 = ay + d[3];
  float* o = p.out + n;
  o[0] = (a0 + b0) / 2.0f * L.stride;
  o[(size_t)p.total] = (a1 + b1) / 2.0f * L.stride;
  o[(size_t)2 * p.total] = (b0 - a0) * L.stride;
  o[(size_t)3 * p.total] = (b1 - a1) * L.stride;
  for (int c0 = 0; c0 < p.nc; c0 += 8) {
    float v[8];
    load8(L.cls, (size_t)pix * L.cls.C + c0, v);
    if (p.scaled) {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] *= L.cls_mul;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (c0 + i < p.nc) o[(size_t)(4 + c0 + i) * p.total] = sigmoid_f(v[i]);
  }
}

hipError_t launch_detect_head_decode(const DetectHeadParams& p, hipStream_t st) {
  int first = 0;
  for (int i = 0; i < 3; ++i) {
    const DetectHeadLevel& L = p.lv[i];
    if (!L.box.hi || !L.cls.hi || L.box.C < 64 || (L.box.C & 7) || (L.cls.C & 7) || L.cls.C < ((p.nc + 7) & ~7) || L.box.H != L.cls.H || L.box.W != L.cls.W || L.first != first ||
        L.box.H < 1 || L.box.W < 1)
      return hipErrorInvalidValue;
    first += L.box.H * L.box.W;
  }
  if (!p.out || p.nc < 1 || p.total != first) return hipErrorInvalidValue;
  VP_LAUNCH(detect_head_decode_kernel, dim3(nblk(p.total)), dim3(256), 0, st, p);
}

// ------------------------------------------------------------------------------------------------ AutoSteer lane rows head
// AutoSteerPerceptHead.forward behind `features` (auto_steer_percept_head.py:58-85), one workgroup per feature row y, one thread per column x (W = 256).
//   conv : (a0, a1) = (c1, c2) biases (BN folded at load); for the taps (ky, kx) in row-major order that lie inside the map, for ci = 0 .. cin - 1:
//          a_o = fmaf(features(y + ky - 1, x + kx - 1, ci) as hi (+ lo), w[tap][ci][o], a_o).  Weights are uniform: LDS, read as broadcasts.
//   lanes: v = SiLU(SiLU(a0)) (Conv's own activation, then :60); m = row maximum; e = expf(v - m); S = sum e, N = sum e * x, both by the same
//          binary tree over the 256 columns in LDS (element t adds element t + s, s = 128, 64, .., 1): xp = N / S / W  (:61-69).
//   height: g = SiLU(SiLU(a1)) (Conv's own activation, then :73); u_j = SiLU(h1_b + g[16 j] * h1_w[0] + .. + g[16 j + 15] * h1_w[15]) for the 16 groups j, each summed in column order by one
//          thread; h = SiLU(h2_b + u_0 * h2_w[0] + .. + u_15 * h2_w[15]) by thread 0  (:72-77).
// No atomics, one fixed order: replays are bit-stable.  The kernel reads 3 x 256 x cin pairs per row (each pixel by three neighbouring threads and
// three rows: L1 / L2 hits) for 2 x 9 x cin FMAs per thread -- 64 workgroups bound by the latency of the loads and of the ten barriers behind them.
__global__ __launch_bounds__(256) void lane_rows_head_kernel(const LaneRowsHeadParams p) {
  __shared__ float sw[9 * 64 * 2];
  __shared__ float red0[256], red1[256], sg[256], su[16];
  const int tid = threadIdx.x, y = blockIdx.x;
  const int H = p.features.H, W = p.features.W, C = p.features.C;
  for (int i = tid; i < 9 * p.cin * 2; i += 256) sw[i] = p.w[i];
  __syncthreads();
  float a0 = p.hw[32], a1 = p.hw[33];
  for (int ky = 0; ky < 3; ++ky) {
    const int yy = y + ky - 1;
    if (yy < 0 || yy >= H) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int xx = tid + kx - 1;
      if (xx < 0 || xx >= W) continue;
      const size_t base = ((size_t)yy * W + xx) * C;
      const float* wt = sw + (ky * 3 + kx) * p.cin * 2;
      for (int c0 = 0; c0 < p.cin; c0 += 8) {
        float v[8];
        load8(p.features, base + c0, v);
        if (p.scaled) {   // VP_ACT_SCALE: true feature values (a power of two times the recombined hi + lo: exact)
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] *= p.in_mul;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          a0 = fmaf(v[j], wt[(c0 + j) * 2], a0);
          a1 = fmaf(v[j], wt[(c0 + j) * 2 + 1], a1);
        }
      }
    }
  }
  const float lane = silu_f(silu_f(a0));
  sg[tid] = silu_f(silu_f(a1));
  red0[tid] = lane;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red0[tid] = fmaxf(red0[tid], red0[tid + s]);
    __syncthreads();
  }
  const float m = red0[0];
  __syncthreads();
  const float e = expf(lane - m);
  red0[tid] = e;
  red1[tid] = e * (float)tid;
  if (tid < 16) {   // height branch, first stage: group tid
    float u = p.hw[34];
    for (int i = 0; i < 16; ++i) u = fmaf(sg[tid * 16 + i], p.hw[i], u);
    su[tid] = silu_f(u);
  }
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      red0[tid] += red0[tid + s];
      red1[tid] += red1[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    // NaN anywhere in the row: fmaxf drops it from m, but expf(NaN - m) carries it into both sums -- the range probe sees it
    p.out[y] = red1[0] / red0[0] / (float)W;
    float h = p.hw[35];
    for (int j = 0; j < 16; ++j) h = fmaf(su[j], p.hw[16 + j], h);
    p.out[H + y] = silu_f(h);
  }
}

bool lane_rows_head_ok(const LaneRowsHeadParams& p) {
  return p.features.hi && p.w && p.hw && p.out && p.features.W == 256 && p.features.H >= 1 && p.features.H <= 65535 && p.cin >= 8 && p.cin <= 64 && !(p.cin & 7) &&
         p.cin <= p.features.C && !(p.features.C & 7);
}
hipError_t launch_lane_rows_head(const LaneRowsHeadParams& p, hipStream_t st) {
  if (!lane_rows_head_ok(p)) return hipErrorInvalidValue;
  VP_LAUNCH(lane_rows_head_kernel, dim3(p.features.H), dim3(256), 0, st, p);
}

// ------------------------------------------------------------------------------------------------ production lane filter (vp_lanes)
// LaneFilter::update's pixel work (VisionPilot/production_release/src/lane_filtering/lane_filter.cpp findStartingPoints :325-369,
// slidingWindowSearch :375-594) on an EgoLanes engine's fp32 logits [3][80][160], one workgroup of four waves per frame:
//   1. the three planes become bit rows in LDS (bit x of row y of plane c: logit > threshold, so a NaN is clear) by LDS atomicOr;
//   2. start points: a thread per row of the lower half finds its row's candidate (left: the highest set x <= 79 of plane 0; right: the lowest set
//      x >= 80 of plane 1), and the bottom-most row that has one wins;
//   3. wave w runs the search of lane w >> 1 in direction w & 1 (0 up, 1 down).  The run's state is wave-uniform: every thread extracts the window's
//      <= 4 rows of <= 12 bits from LDS and derives the counts, the coordinate sums, the float centroid / direction and the next position itself, so no
//      value crosses lanes.  Only the append is spread out: thread p < w * h owns window pixel p (row-major) and stores it at the rank popcount of the
//      set pixels before it gives -- the reference's collection order.
//   4. the moments S_k = sum y^k, T_k = sum x y^k and min / max y are accumulated per run in 64-bit integers and added per lane through LDS.
// The float steps are the host's: IEEE division and square root, dx * dx + dy * dy unfused, roundf for the centroid, truncation for the blind advance.
// A run's y only moves away from its start (the centroid lies inside the window, the direction keeps its sign), so every window lies inside the plane;
// the row range is clamped all the same before LDS is read.
__device__ __forceinline__ unsigned lane_bits_field(const unsigned* row, const int x0, const int ww) {   // bits [x0, x0 + ww) of a bit row, 1 <= ww <= 12
  const int w0 = x0 >> 5, sh = x0 & 31;
  unsigned v = row[w0] >> sh;
  if (sh + ww > 32) v |= row[w0 + 1] << (32 - sh);   // x0 + ww <= 160: word w0 + 1 exists
  return v & ((1u << ww) - 1u);
}
__device__ __forceinline__ int lane_bits_possum(const unsigned v) {   // the sum of the positions of the set bits of a 12-bit field
  return __builtin_popcount(v & 0xAAAu) + 2 * __builtin_popcount(v & 0xCCCu) + 4 * __builtin_popcount(v & 0x0F0u) + 8 * __builtin_popcount(v & 0xF00u);
}

__global__ __launch_bounds__(256) void lane_filter_kernel(const LaneFilterParams p) {
  __shared__ unsigned bits[3 * kLaneH * kLaneRowWords];
  __shared__ int cand[2][kLaneH / 2];
  __shared__ long long s_mom[4][8];
  __shared__ int s_cnt[4][4];
  const int tid = threadIdx.x;
  for (int i = tid; i < 3 * kLaneH * kLaneRowWords; i += 256) bits[i] = 0u;
  __syncthreads();
  // 1. threshold: pixel i of the [3][80][160] tensor is bit i & 31 of word i >> 5 (160 = 5 * 32).  Eight 16-byte loads a thread are in flight at a time
  constexpr int kVec = 3 * kLaneH * kLaneW / 4;
  const float t = p.threshold;
  for (int q0 = tid; q0 < kVec; q0 += 256 * 8) {
    int4 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (q0 + 256 * j < kVec) v[j] = reinterpret_cast<const int4*>(p.logits)[q0 + 256 * j];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int q = q0 + 256 * j;
      if (q < kVec) {
        const unsigned m = (__uint_as_float((unsigned)v[j].x) > t ? 1u : 0u) | (__uint_as_float((unsigned)v[j].y) > t ? 2u : 0u) |
                           (__uint_as_float((unsigned)v[j].z) > t ? 4u : 0u) | (__uint_as_float((unsigned)v[j].w) > t ? 8u : 0u);
        if (m) atomicOr(&bits[q >> 3], m << ((q & 7) * 4));
      }
    }
  }
  __syncthreads();
  // 2. start candidates: thread t of wave 0 / wave 1 takes row 79 - t of the left / right lane
  if ((tid & 63) < kLaneH / 2 && tid < 128) {
    const int side = tid >> 6, y = kLaneH - 1 - (tid & 63);
    const unsigned* row = bits + (side * kLaneH + y) * kLaneRowWords;
    int x = -1;
    if (side == 0) {
      const unsigned w2 = row[2] & 0xFFFFu;   // x 64 .. 79
      if (w2) x = 64 + 31 - __builtin_clz(w2);
      else if (row[1]) x = 32 + 31 - __builtin_clz(row[1]);
      else if (row[0]) x = 31 - __builtin_clz(row[0]);
    } else {
      const unsigned w2 = row[2] & 0xFFFF0000u;   // x 80 .. 95
      if (w2) x = 64 + __builtin_ctz(w2);
      else if (row[3]) x = 96 + __builtin_ctz(row[3]);
      else if (row[4]) x = 128 + __builtin_ctz(row[4]);
    }
    cand[side][tid & 63] = x;
  }
  __syncthreads();
  // 3. the run of this wave
  const int wave = tid >> 6, ln = tid & 63, side = wave >> 1, down = wave & 1;
  int sx = -1, sy = -1;
  for (int r = 0; r < kLaneH / 2; ++r) {
    if (cand[side][r] >= 0) {
      sx = cand[side][r];
      sy = kLaneH - 1 - r;
      break;
    }
  }
  sx = __builtin_amdgcn_readfirstlane(sx);   // wave-uniform by construction: say so, and the run's integer state lives in scalar registers
  sy = __builtin_amdgcn_readfirstlane(sy);
  LaneFilterLane* out = &p.rec->lane[side];
  uint16_t* pts = p.points + (size_t)(side * 2 + down) * kLaneRunPoints;
  const unsigned* ego = bits + side * kLaneH * kLaneRowWords;
  const unsigned* other = bits + 2 * kLaneH * kLaneRowWords;
  int nwin = 0, npts = 0, miny = kLaneH, maxy = -1;
  long long S0 = 0, S1 = 0, S2 = 0, S3 = 0, S4 = 0, T0 = 0, T1 = 0, T2 = 0;
  if (sx >= 0) {
    int x = sx, y = sy + (down ? 4 : 0), empty = 0;
    float dirx = 0.0f, diry = down ? 1.0f : -1.0f;
    for (int step = 0; step < kLaneMaxSteps; ++step) {
      if (x < 0 || x >= kLaneW) break;
      if (down ? y >= kLaneH : y < 0) break;
      const int hw = y < 40 ? 1 : 6;
      const int ylo = down ? y : max(0, y - 4), yhi = down ? min(kLaneH, y + 4) : y;
      const int xlo = max(0, x - hw), xhi = min(kLaneW, x + hw), ww = xhi - xlo;
      if (ln == 0) {
        short* w = out->win[down][nwin];
        w[0] = (short)xlo, w[1] = (short)ylo, w[2] = (short)ww, w[3] = (short)(yhi - ylo);
      }
      ++nwin;
      const bool strict = y < 40;   // above the lower half the other-lane plane is not looked at
      const int r0 = max(ylo, 0), r1 = min(yhi, kLaneH);
      unsigned re[4] = {0u, 0u, 0u, 0u}, ro[4] = {0u, 0u, 0u, 0u};
      int ce = 0, co = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (r0 + r < r1) {
          re[r] = __builtin_amdgcn_readfirstlane(lane_bits_field(ego + (r0 + r) * kLaneRowWords, xlo, ww));
          if (!strict) ro[r] = __builtin_amdgcn_readfirstlane(lane_bits_field(other + (r0 + r) * kLaneRowWords, xlo, ww));
          ce += __builtin_popcount(re[r]);
          co += __builtin_popcount(ro[r]);
        }
      }
      const bool take_ego = ce >= 3, found = take_ego || co >= 3;
      if (found) {
        const int cnt = take_ego ? ce : co;
        unsigned long long m = 0ull;
        unsigned a0 = 0u, a1 = 0u, a2 = 0u, a3 = 0u, a4 = 0u, b0 = 0u, b1 = 0u, b2 = 0u;   // this window's share of the moments: 48 * 79^4 < 2^32
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const unsigned f = take_ego ? re[r] : ro[r];
          const unsigned c = (unsigned)__builtin_popcount(f), yy = (unsigned)(r0 + r), y2 = yy * yy;
          const unsigned xs = c * (unsigned)xlo + (unsigned)lane_bits_possum(f);
          m |= (unsigned long long)f << (r * ww);
          a0 += c, a1 += c * yy, a2 += c * y2, a3 += c * y2 * yy, a4 += c * y2 * y2;
          b0 += xs, b1 += xs * yy, b2 += xs * y2;
          if (c) miny = min(miny, (int)yy), maxy = max(maxy, (int)yy);
        }
        const int sumx = (int)b0, sumy = (int)a1;
        S0 += a0, S1 += a1, S2 += a2, S3 += a3, S4 += a4, T0 += b0, T1 += b1, T2 += b2;
        if (ln < 4 * ww && ((m >> ln) & 1ull)) {
          const int row = (ln >= ww) + (ln >= 2 * ww) + (ln >= 3 * ww), col = ln - row * ww;   // pixel ln of the window, row-major
          const int rank = __builtin_popcountll(m & ((1ull << ln) - 1ull)), at = npts + rank;
          if (at < kLaneRunPoints) pts[at] = (uint16_t)((xlo + col) | ((r0 + row) << 8));
        }
        npts += cnt;
        empty = 0;
        const float cx = __fdiv_rn((float)sumx, (float)cnt), cy = __fdiv_rn((float)sumy, (float)cnt);
        const float dx = __fsub_rn(cx, (float)x), dy = __fsub_rn(cy, (float)y);
        const float len = sqrtf(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
        if (len > 0.1f) {
          dirx = __fdiv_rn(dx, len);
          diry = __fdiv_rn(dy, len);
        }
        x = __builtin_amdgcn_readfirstlane((int)roundf(cx));
        y = __builtin_amdgcn_readfirstlane((int)roundf(cy));
      } else {
        if (!down && y < kLaneH / 4) break;   // the horizon
        if (++empty >= 12) break;
        x += __builtin_amdgcn_readfirstlane((int)__fmul_rn(dirx, 4.0f));      // the blind advance truncates
        y += __builtin_amdgcn_readfirstlane((int)__fmul_rn(diry, 4.0f));
      }
      if (!down && y >= yhi - 1) y -= 4;      // the two forced moves: every step leaves its window
      if (down && y <= ylo + 1) y += 4;
    }
  }
  // 4. per lane: both runs' counts and moments
  if (ln == 0) {
    s_mom[wave][0] = S0, s_mom[wave][1] = S1, s_mom[wave][2] = S2, s_mom[wave][3] = S3, s_mom[wave][4] = S4;
    s_mom[wave][5] = T0, s_mom[wave][6] = T1, s_mom[wave][7] = T2;
    s_cnt[wave][0] = nwin, s_cnt[wave][1] = npts, s_cnt[wave][2] = miny, s_cnt[wave][3] = maxy;
  }
  __syncthreads();
  if (down == 0 && ln < 8) {
    const long long v = s_mom[wave][ln] + s_mom[wave + 1][ln];
    if (ln < 5) out->S[ln] = v;
    else out->T[ln - 5] = v;
    if (ln == 0) {
      out->start_x = sx, out->start_y = sy;
      out->n_windows[0] = s_cnt[wave][0], out->n_windows[1] = s_cnt[wave + 1][0];
      out->n_points[0] = s_cnt[wave][1], out->n_points[1] = s_cnt[wave + 1][1];
      out->min_y = min(s_cnt[wave][2], s_cnt[wave + 1][2]);
      out->max_y = max(s_cnt[wave][3], s_cnt[wave + 1][3]);
    }
  }
}

hipError_t launch_lane_filter(const LaneFilterParams& p, hipStream_t st) {
  if (!p.logits || !p.rec || !p.points || (reinterpret_cast<uintptr_t>(p.logits) & 15)) return hipErrorInvalidValue;
  VP_LAUNCH(lane_filter_kernel, dim3(1), dim3(256), 0, st, p);
}

// ------------------------------------------------------------------------------------------------ validation NMS + matching (vp_metric_add_det*)
// The trainer's validation post-process (Models/training/auto_speed_util.py non_max_suppression :123-169, compute_metric :99-120), as include/vp_hip.h
// defines it; the chain and its buffers: kernels.hpp DetValParams.  Every fp32 operation is one __f*_rn in the order of the definition.
constexpr int kDetRankSlice = 4096, kDetRankTile = 1024, kDetSupThreads = 1024;

// a float's bits, ordered as the floats are (negative scores included: the operator entry takes any tensor); a candidate's is never 0
__device__ __forceinline__ unsigned det_ord(const float s) {
  const unsigned b = __float_as_uint(s);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ __launch_bounds__(256) void det_val_expand_kernel(const DetValParams p) {
  __shared__ unsigned s_n, s_base;
  const unsigned N = p.nb * p.nc, k = blockIdx.x * 256 + threadIdx.x;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  bool cand = false;
  float s = 0.0f;
  if (k < N) {
    const unsigned i = k / p.nc, c = k - i * p.nc;
    s = p.raw[(size_t)(4 + c) * p.nb + i];
    cand = s > p.conf;   // false for a NaN
    p.rank[k] = 0;
  }
  unsigned slot = 0;
  if (cand) slot = atomicAdd(&s_n, 1u);
  __syncthreads();
  if (threadIdx.x == 0 && s_n) s_base = atomicAdd(p.slots, s_n);
  __syncthreads();
  if (cand) p.keys[s_base + slot] = ((unsigned long long)det_ord(s) << 32) | (unsigned long long)(0xFFFFFFFFu - k);
}

// grid (ceil(N / 256), ceil(N / 4096)): the keys [256 x, 256 x + 256) against the slice [4096 y, 4096 y + 4096); workgroups past the count leave
__global__ __launch_bounds__(256) void det_val_rank_kernel(const DetValParams p) {
  __shared__ unsigned long long tile[kDetRankTile];
  const unsigned n = min(*p.slots, p.nb * p.nc), tid = threadIdx.x;
  const unsigned k0 = blockIdx.x * 256, j0 = blockIdx.y * kDetRankSlice;
  if (k0 >= n || j0 >= n) return;
  const unsigned k = k0 + tid, j1 = min(n, j0 + (unsigned)kDetRankSlice);
  const unsigned long long mine = k < n ? p.keys[k] : ~0ull;
  unsigned cnt = 0;
  for (unsigned t = 0; t < kDetRankSlice / kDetRankTile; ++t) {
    const unsigned b = j0 + t * kDetRankTile;
    if (b >= j1) break;   // uniform
    for (unsigned u = tid; u < kDetRankTile; u += 256) tile[u] = b + u < j1 ? p.keys[b + u] : 0ull;
    __syncthreads();
#pragma unroll 8
    for (unsigned u = 0; u < kDetRankTile; ++u) cnt += tile[u] > mine ? 1u : 0u;
    __syncthreads();
  }
  if (k < n && cnt) atomicAdd(&p.rank[k], cnt);
}

// candidate (box i, class c): the corners of wh2xy, and the class offset of the batched NMS
__device__ __forceinline__ f32x4_t det_val_corners(const DetValParams& p, const unsigned i) {
  const float cx = p.raw[i], cy = p.raw[(size_t)p.nb + i], w = p.raw[(size_t)2 * p.nb + i], h = p.raw[(size_t)3 * p.nb + i];
  const float hw = __fdiv_rn(w, 2.0f), hh = __fdiv_rn(h, 2.0f);
  return f32x4_t{__fsub_rn(cx, hw), __fsub_rn(cy, hh), __fadd_rn(cx, hw), __fadd_rn(cy, hh)};
}

__global__ __launch_bounds__(256) void det_val_place_kernel(const DetValParams p) {
  const unsigned n = min(*p.slots, p.nb * p.nc), k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const unsigned r = p.rank[k];
  if (r >= (unsigned)p.max_nms) return;
  const unsigned cand = 0xFFFFFFFFu - (unsigned)(p.keys[k] & 0xFFFFFFFFull);
  const unsigned i = cand / p.nc, c = cand - i * p.nc;
  const f32x4_t b = det_val_corners(p, i);
  const float off = __fmul_rn((float)c, 7680.0f);
  p.order[r] = cand;
  *reinterpret_cast<f32x4_t*>(p.boxes + (size_t)r * 4) = f32x4_t{__fadd_rn(b[0], off), __fadd_rn(b[1], off), __fadd_rn(b[2], off), __fadd_rn(b[3], off)};
}

// One workgroup.  A kept box costs one pass of all threads over the ranks behind it and one barrier; the walk to the next unsuppressed rank is uniform
// (every thread reads the same flags behind the barrier) and skips four suppressed ranks per LDS word.
__global__ __launch_bounds__(kDetSupThreads) void det_val_suppress_kernel(const DetValParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char flags[kDetValMaxNms];
  __shared__ int kept_rank[kDetValMaxDet];
  const int tid = threadIdx.x, n = (int)min(*p.slots, p.nb * p.nc), m = min(n, p.max_nms);
  for (int j = tid; j < m; j += kDetSupThreads) flags[j] = 0;
  __syncthreads();
  int kept = 0, i = 0;
  for (int it = 0; it < p.max_det; ++it) {
    while (i < m) {
      if (!(i & 3) && i + 4 <= m && *reinterpret_cast<const unsigned*>(flags + i) == 0x01010101u) {
        i += 4;
        continue;
      }
      if (!flags[i]) break;
      ++i;
    }
    if (i >= m) break;
    if (tid == 0) kept_rank[kept] = i;
    ++kept;
    if (kept == p.max_det) break;   // the list is full: nothing behind this box is looked at
    const f32x4_t bi = *reinterpret_cast<const f32x4_t*>(p.boxes + (size_t)i * 4);
    // eight boxes per thread and trip, loaded whatever their flags say: the loads of a trip are in flight together (the boxes come from L2)
    for (int j0 = i + 1 + tid; j0 < m; j0 += 8 * kDetSupThreads) {
      f32x4_t bj[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int j = j0 + u * kDetSupThreads;
        bj[u] = j < m ? *reinterpret_cast<const f32x4_t*>(p.boxes + (size_t)j * 4) : f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int j = j0 + u * kDetSupThreads;
        if (j < m && !flags[j] && det_iou<true>(bi, bj[u]) > p.iou) flags[j] = 1;
      }
    }
    __syncthreads();
    ++i;
  }
  __syncthreads();
  for (int t = tid; t < kept; t += kDetSupThreads) {
    const unsigned cand = p.order[kept_rank[t]];
    const unsigned bi = cand / p.nc, c = cand - bi * p.nc;
    const f32x4_t b = det_val_corners(p, bi);
    float* o = p.rows + (size_t)t * kDetValRowWords;
    o[0] = b[0];
    o[1] = b[1];
    o[2] = b[2];
    o[3] = b[3];
    o[4] = p.raw[(size_t)(4 + c) * p.nb + bi];
    o[5] = (float)c;
    o[6] = 0.0f;   // the tp word: no bit
  }
  if (tid == 0) {
    p.counts[0] = (unsigned)n;
    p.counts[1] = (unsigned)m;
    p.counts[2] = (unsigned)kept;
  }
}

size_t det_val_scratch_bytes(const unsigned nb, const unsigned nc) {
  const size_t N = (size_t)nb * nc, m = N < (size_t)kDetValMaxNms ? N : (size_t)kDetValMaxNms;
  const auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  return 256 + up(8 * N) + up(4 * N) + up(4 * m) + up(16 * m);
}

void det_val_carve(uint8_t* s, DetValParams* p) {
  const size_t N = (size_t)p->nb * p->nc, m = N < (size_t)kDetValMaxNms ? N : (size_t)kDetValMaxNms;
  const auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  p->slots = reinterpret_cast<unsigned*>(s);
  p->keys = reinterpret_cast<unsigned long long*>(s + 256);
  p->rank = reinterpret_cast<unsigned*>(s + 256 + up(8 * N));
  p->order = reinterpret_cast<unsigned*>(s + 256 + up(8 * N) + up(4 * N));
  p->boxes = reinterpret_cast<float*>(s + 256 + up(8 * N) + up(4 * N) + up(4 * m));
}

bool det_val_ok(const DetValParams& p) {
  return p.raw && p.slots && p.keys && p.rank && p.order && p.boxes && p.rows && p.counts && p.nc >= 1 && p.nc <= (unsigned)kDetValMaxClasses && p.nb >= 1 &&
         p.nb <= (unsigned)kDetValMaxBoxes && (unsigned long long)p.nb * p.nc <= (unsigned long long)kDetValMaxPairs && p.max_nms >= 1 && p.max_nms <= kDetValMaxNms &&
         p.max_det >= 1 && p.max_det <= kDetValMaxDet && !(reinterpret_cast<uintptr_t>(p.boxes) & 15) && !(reinterpret_cast<uintptr_t>(p.keys) & 7);
}

hipError_t launch_det_validate(const DetValParams& p, hipStream_t st) {
  if (!det_val_ok(p)) return hipErrorInvalidValue;
  const unsigned N = p.nb * p.nc, gx = nblk(N), gy = (N + kDetRankSlice - 1) / kDetRankSlice;
  if (hipError_t e = hipMemsetAsync(p.slots, 0, sizeof(unsigned), st); e != hipSuccess) return e;
  hipLaunchKernelGGL(det_val_expand_kernel, dim3(gx), dim3(256), 0, st, p);
  hipLaunchKernelGGL(det_val_rank_kernel, dim3(gx, gy), dim3(256), 0, st, p);
  hipLaunchKernelGGL(det_val_place_kernel, dim3(gx), dim3(256), 0, st, p);
  VP_LAUNCH(det_val_suppress_kernel, dim3(1), dim3(kDetSupThreads), 0, st, p);
}

// pair form: the reference chain's kept rows with score > label_conf, in order, as label rows in pixels
__global__ __launch_bounds__(256) void det_val_labels_kernel(const DetValLabelsParams p) {
  __shared__ int flag[kDetValMaxDet];
  const int tid = threadIdx.x, kept = (int)min(p.counts[2], (unsigned)kDetValMaxDet);
  for (int d = tid; d < kept; d += 256) flag[d] = p.rows[(size_t)d * kDetValRowWords + 4] > p.label_conf ? 1 : 0;
  __syncthreads();
  for (int d = tid; d < kept; d += 256) {
    if (!flag[d]) continue;
    int pos = 0;
    for (int e = 0; e < d; ++e) pos += flag[e];
    const float* r = p.rows + (size_t)d * kDetValRowWords;
    float* o = p.labels + (size_t)pos * 5;
    o[0] = r[5];
    o[1] = r[0];
    o[2] = r[1];
    o[3] = r[2];
    o[4] = r[3];
  }
  if (tid == 0) {
    int total = 0;
    for (int e = 0; e < kept; ++e) total += flag[e];
    *p.n_labels = (unsigned)total;
  }
}

hipError_t launch_det_val_labels(const DetValLabelsParams& p, hipStream_t st) {
  if (!p.rows || !p.counts || !p.labels || !p.n_labels) return hipErrorInvalidValue;
  VP_LAUNCH(det_val_labels_kernel, dim3(1), dim3(256), 0, st, p);
}

// torch.min / torch.max / clamp(0) hand a NaN on (fminf / fmaxf would drop it)
__device__ __forceinline__ float det_min_nan(const float a, const float b) { return (a != a || b != b) ? __uint_as_float(0x7FC00000u) : fminf(a, b); }
__device__ __forceinline__ float det_max_nan(const float a, const float b) { return (a != a || b != b) ? __uint_as_float(0x7FC00000u) : fmaxf(a, b); }

__device__ __forceinline__ f32x4_t det_val_label_box(const DetMatchParams& p, const float* l) {
  if (p.label_form) return f32x4_t{l[1], l[2], l[3], l[4]};
  const float hw = __fdiv_rn(l[3], 2.0f), hh = __fdiv_rn(l[4], 2.0f);
  return f32x4_t{__fmul_rn(__fsub_rn(l[1], hw), p.W), __fmul_rn(__fsub_rn(l[2], hh), p.H), __fmul_rn(__fadd_rn(l[1], hw), p.W), __fmul_rn(__fadd_rn(l[2], hh), p.H)};
}

// compute_metric (:99-120).  The best label of a detection is its same-class label of highest IoU (the first of equals), whatever the threshold: at
// threshold t the detection is eligible when that IoU >= t.  Among the eligible detections that share a best label the one of LOWEST index is correct
// (what the two numpy.unique(..., return_index=True) calls leave).
__global__ __launch_bounds__(256) void det_val_match_kernel(const DetMatchParams p) {
  __shared__ float best_iou[kDetValMaxDet];
  __shared__ int best_lab[kDetValMaxDet];
  const int tid = threadIdx.x, kept = (int)min(p.counts[2], (unsigned)kDetValMaxDet);
  const int nl = p.n_labels_dev ? (int)min(*p.n_labels_dev, (unsigned)p.n_labels) : p.n_labels;
  const unsigned row0 = p.totals[0], lab0 = p.totals[1];
  for (int d = tid; d < kept; d += 256) {
    const float* r = p.rows + (size_t)d * kDetValRowWords;
    const float area_d = __fmul_rn(__fsub_rn(r[2], r[0]), __fsub_rn(r[3], r[1]));
    float best = 0.0f;
    int lab = -1;
    for (int l = 0; l < nl; ++l) {
      const float* L = p.labels + (size_t)l * 5;
      if (!(L[0] == r[5])) continue;
      const f32x4_t a = det_val_label_box(p, L);
      float iw = __fsub_rn(det_min_nan(a[2], r[2]), det_max_nan(a[0], r[0]));
      float ih = __fsub_rn(det_min_nan(a[3], r[3]), det_max_nan(a[1], r[1]));
      iw = iw < 0.0f ? 0.0f : iw;
      ih = ih < 0.0f ? 0.0f : ih;
      const float inter = __fmul_rn(iw, ih);
      const float area_l = __fmul_rn(__fsub_rn(a[2], a[0]), __fsub_rn(a[3], a[1]));
      const float iou = __fdiv_rn(inter, __fadd_rn(__fsub_rn(__fadd_rn(area_l, area_d), inter), 1e-7f));
      if (iou == iou && (lab < 0 || iou > best)) {
        best = iou;
        lab = l;
      }
    }
    best_iou[d] = best;
    best_lab[d] = lab;
  }
  __syncthreads();
  for (int d = tid; d < kept; d += 256) {
    unsigned tp = 0;
    const int lab = best_lab[d];
    if (lab >= 0) {
      for (int t = 0; t < p.n_iou; ++t) {
        bool ok = best_iou[d] >= p.iou_v[t];
        for (int e = 0; e < d && ok; ++e) ok = !(best_lab[e] == lab && best_iou[e] >= p.iou_v[t]);
        tp |= ok ? 1u << t : 0u;
      }
    }
    const float* r = p.rows + (size_t)d * kDetValRowWords;
    DetRowRecord o;
    o.x1 = r[0];
    o.y1 = r[1];
    o.x2 = r[2];
    o.y2 = r[3];
    o.conf = r[4];
    o.cls = r[5];
    o.tp = tp;
    p.rows_out[(size_t)row0 + d] = o;
  }
  for (int l = tid; l < nl; l += 256) p.label_cls_out[(size_t)lab0 + l] = p.labels[(size_t)l * 5];
  if (tid == 0) {
    DetFrameRecord f;
    f.candidates = p.counts[0];
    f.ranked = p.counts[1];
    f.kept = (unsigned)kept;
    f.labels = (unsigned)nl;
    f.first_row = row0;
    *p.frame = f;
  }
  __syncthreads();   // every thread has read the totals
  if (tid == 0) {
    p.totals[0] = row0 + (unsigned)kept;
    p.totals[1] = lab0 + (unsigned)nl;
  }
}

hipError_t launch_det_val_match(const DetMatchParams& p, hipStream_t st) {
  if (!p.rows || !p.counts || (p.n_labels > 0 && !p.labels) || p.n_labels < 0 || p.n_labels > kDetValMaxLabels || p.n_iou < 1 || p.n_iou > kDetValMaxIou || !p.totals ||
      !p.frame || !p.rows_out || !p.label_cls_out)
    return hipErrorInvalidValue;
  VP_LAUNCH(det_val_match_kernel, dim3(1), dim3(256), 0, st, p);
}

}  // namespace vp

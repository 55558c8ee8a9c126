// vp_detect_*: the AutoSpeed detector's letterbox preprocess and decode + NMS on the device behind the C ABI (include/vp_hip.h; SURVEY.md N4;
// VisionPilot/middleware_recipes/common/backends/autospeed/onnxruntime_engine.cpp:71-113, :170-290).  The detector network is a VP_AUTOSPEED
// engine (engine.cpp build_autospeed) attached with vp_detect_attach: vp_detect_infer runs frame -> detections without leaving the device.  The
// two-call form (a host's own runtime between vp_detect_preprocess and vp_detect_postprocess) stays as it was.
// vp_detect_preprocess_pil / _postprocess_agnostic / _infer_pil: the same three entries in the arithmetic of the Python wrapper
// (Models/inference/auto_speed_infer.py), which letterboxes with Pillow and decodes differently; they share the handle, its buffers and its stored geometry.
#include <cmath>
#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/vp_hip.h"
#include "engine.hpp"
#include "vp_handle.hpp"
#include "kernels.hpp"

static_assert(sizeof(vp_detection) == sizeof(vp::Detection) && sizeof(vp_detection) == 24, "vp_detection is the reference's Detection");

struct vp_detect {
  int gpu = 0, net_h = 0, net_w = 0, max_boxes = 0, max_attrs = 0;
  hipStream_t stream = nullptr;
  uint8_t* d_frame = nullptr;
  size_t frame_cap = 0;
  uint8_t* h_frame = nullptr;  // pinned staging
  size_t h_frame_cap = 0;
  int* d_xtab = nullptr;
  int* d_ytab = nullptr;
  int tab_w = 0, tab_h = 0, tab_cap_w = 0, tab_cap_h = 0;
  float* d_input = nullptr;  // [3][net_h][net_w]
  float* d_raw = nullptr;    // [max_attrs][max_boxes]
  float* d_boxes = nullptr;
  int* d_cls = nullptr;
  vp::Detection* d_out = nullptr;
  int* d_count = nullptr;
  vp::Detection* h_out = nullptr;  // pinned [max_boxes]
  int* h_count = nullptr;          // pinned [2]
  // letterbox geometry of the last preprocessed frame (scale_, pad_x_, pad_y_, orig_width_, orig_height_ of the reference engine)
  float scale = 0.0f;
  int pad_x = 0, pad_y = 0, orig_w = 0, orig_h = 0;
  // Pillow letterbox (vp_detect_preprocess_pil): the tables of vp_resample_coeffs for the last frame size, Pillow's u8 image between its two passes,
  // the resized fp32 planes the paste kernel reads
  int* d_pil_tab[4] = {nullptr, nullptr, nullptr, nullptr};   // hb, hk, vb, vk
  int pil_hks = 0, pil_vks = 0, pil_w = 0, pil_h = 0;
  uint8_t* d_pil_tmp = nullptr;
  size_t pil_tmp_cap = 0;
  float* d_pil_planes = nullptr;   // [3][new_h][new_w], room for [3][net_h][net_w]
  std::string err;
  vp_engine* net = nullptr;        // borrowed VP_AUTOSPEED engine (vp_detect_attach)
  hipEvent_t ev_in = nullptr, ev_out = nullptr;   // input tensor written (detector stream -> engine stream), network done (engine -> detector)

  ~vp_detect() {
    (void)hipSetDevice(gpu);
    if (stream) (void)hipStreamSynchronize(stream);
    for (void* q : {(void*)d_frame, (void*)d_xtab, (void*)d_ytab, (void*)d_input, (void*)d_raw, (void*)d_boxes, (void*)d_cls, (void*)d_out, (void*)d_count,
                    (void*)d_pil_tab[0], (void*)d_pil_tab[1], (void*)d_pil_tab[2], (void*)d_pil_tab[3], (void*)d_pil_tmp, (void*)d_pil_planes})
      if (q) (void)hipFree(q);
    for (void* q : {(void*)h_frame, (void*)h_out, (void*)h_count})
      if (q) (void)hipHostFree(q);
    if (ev_in) (void)hipEventDestroy(ev_in);
    if (ev_out) (void)hipEventDestroy(ev_out);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace {

void set_err(char* err, size_t n, const std::string& msg) {
  if (err && n) {
    std::strncpy(err, msg.c_str(), n - 1);
    err[n - 1] = 0;
  }
}

template <class F>
int guarded(vp_detect* d, F&& f) {
  if (!d) return VP_ERR_ARG;
  try {
    VP_HIP_CHECK(hipSetDevice(d->gpu));
    return f();
  } catch (const std::invalid_argument& ex) {
    d->err = ex.what();
    return VP_ERR_ARG;
  } catch (const std::exception& ex) {
    d->err = ex.what();
    return VP_ERR_HIP;
  }
}

}  // namespace

extern "C" {

int vp_detect_create(vp_detect** out, int gpu_id, int net_h, int net_w, int max_boxes, int max_attrs, char* err, size_t err_len) {
  if (!out || net_h < 1 || net_w < 1 || net_h > 8192 || net_w > 8192 || max_boxes < 1 || max_boxes > vp::kDetectMaxBoxes || max_attrs < 5 || max_attrs > 4096) {
    set_err(err, err_len, "vp_detect_create: bad argument (max_boxes <= 16384, max_attrs >= 5)");
    return VP_ERR_ARG;
  }
  try {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) throw std::runtime_error("no HIP device visible: the detector stages have no CPU fallback");
    if (gpu_id < 0 || gpu_id >= n) throw std::invalid_argument("gpu_id out of range");
    auto d = std::make_unique<vp_detect>();
    d->gpu = gpu_id;
    d->net_h = net_h;
    d->net_w = net_w;
    d->max_boxes = max_boxes;
    d->max_attrs = max_attrs;
    VP_HIP_CHECK(hipSetDevice(gpu_id));
    VP_HIP_CHECK(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
    VP_HIP_CHECK(hipMalloc(&d->d_input, (size_t)3 * net_h * net_w * sizeof(float)));
    VP_HIP_CHECK(hipMalloc(&d->d_raw, (size_t)max_attrs * max_boxes * sizeof(float)));
    VP_HIP_CHECK(hipMalloc(&d->d_boxes, (size_t)max_boxes * 4 * sizeof(float)));
    VP_HIP_CHECK(hipMalloc(&d->d_cls, (size_t)max_boxes * sizeof(int)));
    VP_HIP_CHECK(hipMalloc(&d->d_out, (size_t)max_boxes * sizeof(vp::Detection)));
    VP_HIP_CHECK(hipMalloc(&d->d_count, 2 * sizeof(int)));
    VP_HIP_CHECK(hipHostMalloc(&d->h_out, (size_t)max_boxes * sizeof(vp::Detection)));
    VP_HIP_CHECK(hipHostMalloc(&d->h_count, 2 * sizeof(int)));
    *out = d.release();
    return VP_OK;
  } catch (const std::invalid_argument& ex) {
    set_err(err, err_len, ex.what());
    return VP_ERR_ARG;
  } catch (const std::exception& ex) {
    set_err(err, err_len, ex.what());
    return VP_ERR_HIP;
  }
}

void vp_detect_destroy(vp_detect* d) { delete d; }

const char* vp_detect_last_error(const vp_detect* d) { return d ? d->err.c_str() : "null handle"; }

}  // extern "C"

namespace {
// the frame's bytes into d->d_frame through the pinned staging buffer, on the detector's stream (both grown on demand)
void upload_frame(vp_detect* d, const uint8_t* bgr, int h, int w, int stride_bytes) {
    const size_t bytes = (size_t)(h - 1) * stride_bytes + (size_t)3 * w;   // a strided view may END with its last pixel: never read a full last stride
    if (bytes > d->frame_cap) {
      if (d->d_frame) VP_HIP_CHECK(hipFree(d->d_frame));
      d->d_frame = nullptr;
      d->frame_cap = 0;
      VP_HIP_CHECK(hipMalloc(&d->d_frame, bytes));
      d->frame_cap = bytes;
    }
    if (bytes > d->h_frame_cap) {
      if (d->h_frame) VP_HIP_CHECK(hipHostFree(d->h_frame));
      d->h_frame = nullptr;
      d->h_frame_cap = 0;
      VP_HIP_CHECK(hipHostMalloc(&d->h_frame, bytes));
      d->h_frame_cap = bytes;
    }
    VP_HIP_CHECK(hipStreamSynchronize(d->stream));  // the staging buffer and the tables must not be rewritten under a copy still in flight (a drained stream: no wait)
    std::memcpy(d->h_frame, bgr, bytes);
    VP_HIP_CHECK(hipMemcpyAsync(d->d_frame, d->h_frame, bytes, hipMemcpyHostToDevice, d->stream));
}

// upload + letterbox of one frame into `dst` ([3][net_h][net_w] fp32) on the detector's stream; no synchronisation behind the launch.  `who`: the
// entry point named in error texts.  Two waits on the detector's own stream, neither of which blocks in steady state: the one ahead of the staging
// copy finds the stream drained (every entry returns synchronised), and the one behind the tap tables runs only when the frame size changes.
void letterbox_frame(vp_detect* d, const char* who, const uint8_t* bgr, int h, int w, int stride_bytes, float* dst) {
    if (!bgr || h < 1 || w < 1 || h > 16384 || w > 16384 || stride_bytes < 3 * w) throw std::invalid_argument(std::string(who) + ": bad frame geometry");
    // preprocessAutoSpeed :78-98 -- fp32 scale, truncated new size, centred paste
    const float scale = std::min((float)d->net_w / (float)w, (float)d->net_h / (float)h);
    const int new_w = (int)((float)w * scale), new_h = (int)((float)h * scale);
    if (new_w < 1 || new_h < 1 || new_w > d->net_w || new_h > d->net_h) throw std::invalid_argument(std::string(who) + ": the frame collapses under the letterbox scale");
    upload_frame(d, bgr, h, w, stride_bytes);
    if (d->tab_w != w || d->tab_h != h) {
      std::vector<int> xt, yt;
      vp::linear_taps_u8(w, new_w, &xt);
      vp::linear_taps_u8(h, new_h, &yt);
      if (new_w > d->tab_cap_w) {
        if (d->d_xtab) VP_HIP_CHECK(hipFree(d->d_xtab));
        d->d_xtab = nullptr;
        VP_HIP_CHECK(hipMalloc(&d->d_xtab, (size_t)d->net_w * 4 * sizeof(int)));
        d->tab_cap_w = d->net_w;
      }
      if (new_h > d->tab_cap_h) {
        if (d->d_ytab) VP_HIP_CHECK(hipFree(d->d_ytab));
        d->d_ytab = nullptr;
        VP_HIP_CHECK(hipMalloc(&d->d_ytab, (size_t)d->net_h * 4 * sizeof(int)));
        d->tab_cap_h = d->net_h;
      }
      // on the detector's own stream, then waited for: hipMemcpy would use the legacy stream, which the runtime refuses while any thread captures a graph
      VP_HIP_CHECK(hipMemcpyAsync(d->d_xtab, xt.data(), xt.size() * sizeof(int), hipMemcpyHostToDevice, d->stream));
      VP_HIP_CHECK(hipMemcpyAsync(d->d_ytab, yt.data(), yt.size() * sizeof(int), hipMemcpyHostToDevice, d->stream));
      VP_HIP_CHECK(hipStreamSynchronize(d->stream));
      d->tab_w = w;
      d->tab_h = h;
    }
    vp::LetterboxParams p{};
    p.frame = d->d_frame;
    p.stride = stride_bytes;
    p.xtab = d->d_xtab;
    p.ytab = d->d_ytab;
    p.new_w = new_w;
    p.new_h = new_h;
    p.pad_x = (d->net_w - new_w) / 2;
    p.pad_y = (d->net_h - new_h) / 2;
    p.out_h = d->net_h;
    p.out_w = d->net_w;
    p.out = dst;
    VP_HIP_CHECK(vp::launch_letterbox(p, d->stream));
    d->scale = scale;
    d->pad_x = p.pad_x;
    d->pad_y = p.pad_y;
    d->orig_w = w;
    d->orig_h = h;
}

// resize_letterbox of the Python wrapper (auto_speed_infer.py:24-34) in the doubles Python computes it in: scale = min(tw / ow, th / oh),
// new = int(o * scale) (truncated), pad = (t - new) // 2.  False when the resized image would be empty (Pillow refuses it too).
#pragma clang fp contract(off)
bool pil_geometry(int net_h, int net_w, int h, int w, double* scale, int* new_w, int* new_h, int* pad_x, int* pad_y) {
  const double s = std::min((double)net_w / (double)w, (double)net_h / (double)h);
  const int nw = (int)((double)w * s), nh = (int)((double)h * s);
  if (nw < 1 || nh < 1 || nw > net_w || nh > net_h) return false;
  *scale = s;
  *new_w = nw;
  *new_h = nh;
  *pad_x = (net_w - nw) / 2;   // never negative: / is //
  *pad_y = (net_h - nh) / 2;
  return true;
}

// upload + Pillow letterbox of one frame into `dst` ([3][net_h][net_w] fp32) on the detector's stream, no synchronisation behind the launches: Pillow's
// two passes (launch_pil_resample on the tables of vp_resample_coeffs, BILINEAR) into d_pil_planes, then the paste.  Waits as letterbox_frame.
void letterbox_pil_frame(vp_detect* d, const char* who, const uint8_t* frame, int h, int w, int stride_bytes, int pixel_format, float* dst) {
  if (!frame || h < 1 || w < 1 || h > 16384 || w > 16384 || stride_bytes < 3 * w) throw std::invalid_argument(std::string(who) + ": bad frame geometry");
  if (pixel_format != VP_BGR8 && pixel_format != VP_RGB8) throw std::invalid_argument(std::string(who) + ": pixel_format is VP_BGR8 or VP_RGB8");
  double scale = 0.0;
  int new_w = 0, new_h = 0, pad_x = 0, pad_y = 0;
  if (!pil_geometry(d->net_h, d->net_w, h, w, &scale, &new_w, &new_h, &pad_x, &pad_y))
    throw std::invalid_argument(std::string(who) + ": the frame collapses under the letterbox scale");
  upload_frame(d, frame, h, w, stride_bytes);
  if (!d->d_pil_planes) VP_HIP_CHECK(hipMalloc(&d->d_pil_planes, (size_t)3 * d->net_h * d->net_w * sizeof(float)));
  if (d->pil_w != w || d->pil_h != h) {
    std::vector<int> tab[4];
    const int hks = vp::pil_coeffs(w, new_w, 1, &tab[0], &tab[1]), vks = vp::pil_coeffs(h, new_h, 1, &tab[2], &tab[3]);
    d->pil_w = d->pil_h = 0;
    for (int i = 0; i < 4; ++i) {   // once per frame size: the tap count follows the size, so the tables are simply made anew
      if (d->d_pil_tab[i]) VP_HIP_CHECK(hipFree(d->d_pil_tab[i]));
      d->d_pil_tab[i] = nullptr;
      VP_HIP_CHECK(hipMalloc(&d->d_pil_tab[i], tab[i].size() * sizeof(int)));
      VP_HIP_CHECK(hipMemcpyAsync(d->d_pil_tab[i], tab[i].data(), tab[i].size() * sizeof(int), hipMemcpyHostToDevice, d->stream));
    }
    const size_t tmp_bytes = (size_t)h * new_w * 3;
    if (tmp_bytes > d->pil_tmp_cap) {
      if (d->d_pil_tmp) VP_HIP_CHECK(hipFree(d->d_pil_tmp));
      d->d_pil_tmp = nullptr;
      d->pil_tmp_cap = 0;
      VP_HIP_CHECK(hipMalloc(&d->d_pil_tmp, tmp_bytes));
      d->pil_tmp_cap = tmp_bytes;
    }
    VP_HIP_CHECK(hipStreamSynchronize(d->stream));   // the host vectors leave scope
    d->pil_hks = hks;
    d->pil_vks = vks;
    d->pil_w = w;
    d->pil_h = h;
  }
  vp::PilResampleParams q{};
  q.frame = d->d_frame;
  q.stride = stride_bytes;
  q.in_h = h;
  q.in_w = w;
  q.out_h = new_h;
  q.out_w = new_w;
  q.hb = d->d_pil_tab[0];
  q.hk = d->d_pil_tab[1];
  q.hks = d->pil_hks;
  q.vb = d->d_pil_tab[2];
  q.vk = d->d_pil_tab[3];
  q.vks = d->pil_vks;
  q.tmp = d->d_pil_tmp;
  for (int c = 0; c < 3; ++c) {
    q.src_c[c] = pixel_format == VP_RGB8 ? c : 2 - c;   // planes R, G, B
    q.mean[c] = 0.0f;                                    // (u8 / 255 - 0) / 1: ToTensor's value, exactly
    q.stdv[c] = 1.0f;
  }
  q.out = d->d_pil_planes;
  q.norm_form = 0;
  VP_HIP_CHECK(vp::launch_pil_resample(q, d->stream));
  vp::LetterboxPasteParams p{};
  p.src = d->d_pil_planes;
  p.new_w = new_w;
  p.new_h = new_h;
  p.pad_x = pad_x;
  p.pad_y = pad_y;
  p.out_h = d->net_h;
  p.out_w = d->net_w;
  p.out = dst;
  VP_HIP_CHECK(vp::launch_letterbox_paste(p, d->stream));
  d->scale = (float)scale;
  d->pad_x = pad_x;
  d->pad_y = pad_y;
  d->orig_w = w;
  d->orig_h = h;
}

vp::DetectAgnosticParams agnostic_params(vp_detect* d, const float* raw, int num_attrs, int num_boxes, float conf_thresh, float iou_thresh, int out_cap) {
  vp::DetectAgnosticParams p{};
  p.raw = raw;
  p.num_attrs = num_attrs;
  p.num_boxes = num_boxes;
  p.conf_thresh = conf_thresh;
  p.iou_thresh = iou_thresh;
  p.scale = d->scale;
  p.pad_x = d->pad_x;
  p.pad_y = d->pad_y;
  p.orig_w = d->orig_w;
  p.orig_h = d->orig_h;
  p.boxes = d->d_boxes;
  p.cls = d->d_cls;
  p.out = reinterpret_cast<float*>(d->d_out);   // [max_boxes] rows of 24 bytes either way
  p.out_cap = std::min(out_cap, d->max_boxes);
  p.count = d->d_count;
  return p;
}
}  // namespace

extern "C" {

int vp_detect_preprocess(vp_detect* d, const uint8_t* bgr, int h, int w, int stride_bytes, float* dst_host_chw) {
  return guarded(d, [&]() -> int {
    letterbox_frame(d, "vp_detect_preprocess", bgr, h, w, stride_bytes, d->d_input);
    if (dst_host_chw) VP_HIP_CHECK(hipMemcpyAsync(dst_host_chw, d->d_input, (size_t)3 * d->net_h * d->net_w * sizeof(float), hipMemcpyDeviceToHost, d->stream));
    VP_HIP_CHECK(hipStreamSynchronize(d->stream));
    return VP_OK;
  });
}

int vp_detect_input_device(const vp_detect* d, void** dev_f32_chw) {
  if (!d || !dev_f32_chw) return VP_ERR_ARG;
  *dev_f32_chw = d->d_input;
  return VP_OK;
}

int vp_detect_letterbox(const vp_detect* d, float* scale, int* pad_x, int* pad_y) {
  if (!d || d->orig_w == 0) return VP_ERR_ARG;
  if (scale) *scale = d->scale;
  if (pad_x) *pad_x = d->pad_x;
  if (pad_y) *pad_y = d->pad_y;
  return VP_OK;
}

int vp_detect_set_letterbox(vp_detect* d, float scale, int pad_x, int pad_y, int orig_w, int orig_h) {
  if (!d || !(scale > 0.0f) || orig_w < 1 || orig_h < 1) return VP_ERR_ARG;
  d->scale = scale;
  d->pad_x = pad_x;
  d->pad_y = pad_y;
  d->orig_w = orig_w;
  d->orig_h = orig_h;
  return VP_OK;
}

int vp_detect_postprocess(vp_detect* d, const float* raw, int raw_on_device, int num_attrs, int num_boxes, float conf_thresh, float iou_thresh,
                          vp_detection* out, int out_cap, int* count) {
  return guarded(d, [&]() -> int {
    if (!raw || !count || out_cap < 0 || (out_cap > 0 && !out) || num_attrs < 5 || num_attrs > d->max_attrs || num_boxes < 1 || num_boxes > d->max_boxes)
      throw std::invalid_argument("vp_detect_postprocess: bad argument (num_attrs / num_boxes within the sizes given to vp_detect_create)");
    if (d->orig_w == 0) throw std::invalid_argument("vp_detect_postprocess: no letterbox geometry yet (vp_detect_preprocess or vp_detect_set_letterbox first)");
    const float* src = raw;
    if (!raw_on_device) {
      VP_HIP_CHECK(hipMemcpyAsync(d->d_raw, raw, (size_t)num_attrs * num_boxes * sizeof(float), hipMemcpyHostToDevice, d->stream));
      src = d->d_raw;
    }
    vp::DetectParams p{};
    p.raw = src;
    p.num_attrs = num_attrs;
    p.num_boxes = num_boxes;
    p.conf_thresh = conf_thresh;
    p.iou_thresh = iou_thresh;
    p.scale = d->scale;
    p.pad_x = d->pad_x;
    p.pad_y = d->pad_y;
    p.orig_w = d->orig_w;
    p.orig_h = d->orig_h;
    p.boxes = d->d_boxes;
    p.cls = d->d_cls;
    p.out = d->d_out;
    p.out_cap = std::min(out_cap, d->max_boxes);
    p.count = d->d_count;
    VP_HIP_CHECK(vp::launch_detect_decode_nms(p, d->stream));
    VP_HIP_CHECK(hipMemcpyAsync(d->h_count, d->d_count, 2 * sizeof(int), hipMemcpyDeviceToHost, d->stream));
    VP_HIP_CHECK(hipStreamSynchronize(d->stream));
    const int kept = d->h_count[0], n = std::min(kept, p.out_cap);
    if (n > 0) {
      VP_HIP_CHECK(hipMemcpyAsync(d->h_out, d->d_out, (size_t)n * sizeof(vp::Detection), hipMemcpyDeviceToHost, d->stream));
      VP_HIP_CHECK(hipStreamSynchronize(d->stream));
      std::memcpy(out, d->h_out, (size_t)n * sizeof(vp::Detection));
    }
    *count = kept;
    return VP_OK;
  });
}

int vp_detect_attach(vp_detect* d, vp_engine* net) {
  return guarded(d, [&]() -> int {
    if (!net) {
      d->net = nullptr;
      return VP_OK;
    }
    if (!net->impl || net->impl->kind() != 5) throw std::invalid_argument("vp_detect_attach: the engine is not a VP_AUTOSPEED engine");
    vp::Engine& g = *net->impl;
    if (g.gpu() != d->gpu) throw std::invalid_argument("vp_detect_attach: the engine lives on GPU " + std::to_string(g.gpu()) + ", the detector on GPU " + std::to_string(d->gpu));
    if (d->net_h != g.net_h() || d->net_w != g.net_w())
      throw std::invalid_argument("vp_detect_attach: the detector was created for a " + std::to_string(d->net_h) + " x " + std::to_string(d->net_w) + " input, the network takes " +
                                  std::to_string(g.net_h()) + " x " + std::to_string(g.net_w()));
    if (d->max_boxes < g.out_w() || d->max_attrs < g.out_c())
      throw std::invalid_argument("vp_detect_attach: the network's output is [" + std::to_string(g.out_c()) + "][" + std::to_string(g.out_w()) + "]: create the detector with max_attrs >= " +
                                  std::to_string(g.out_c()) + " and max_boxes >= " + std::to_string(g.out_w()));
    if (!d->ev_in) VP_HIP_CHECK(hipEventCreateWithFlags(&d->ev_in, hipEventDisableTiming));
    if (!d->ev_out) VP_HIP_CHECK(hipEventCreateWithFlags(&d->ev_out, hipEventDisableTiming));
    d->net = net;
    return VP_OK;
  });
}

int vp_detect_infer(vp_detect* d, const uint8_t* bgr, int h, int w, int stride_bytes, float conf_thresh, float iou_thresh, vp_detection* out, int out_cap,
                    int* count) {
  return guarded(d, [&]() -> int {
    if (!d->net || !d->net->impl) throw std::invalid_argument("vp_detect_infer: no network attached (vp_detect_attach with a VP_AUTOSPEED engine first)");
    if (!count || out_cap < 0 || (out_cap > 0 && !out)) throw std::invalid_argument("vp_detect_infer: bad output arguments");
    vp::Engine& g = *d->net->impl;
    try {
     try {
      // letterbox straight into the network's input tensor: every exit of this call, the failing ones included (see the handler below), leaves both
      // streams drained, so nothing still reads it
      letterbox_frame(d, "vp_detect_infer", bgr, h, w, stride_bytes, g.dev_input());
      g.note_device_tensor();
      VP_HIP_CHECK(hipEventRecord(d->ev_in, d->stream));
      VP_HIP_CHECK(hipStreamWaitEvent(g.stream(), d->ev_in, 0));
      g.enqueue();         // the replayed graph (first call: the eager warm-up pass)
      g.enqueue_status_fetch();   // the range probe's verdict behind it; the output tensor itself stays on the device
      VP_HIP_CHECK(hipEventRecord(d->ev_out, g.stream()));
      VP_HIP_CHECK(hipStreamWaitEvent(d->stream, d->ev_out, 0));
      vp::DetectParams p{};
      p.raw = static_cast<const float*>(g.dev_logits());
      p.num_attrs = g.out_c();
      p.num_boxes = g.out_w();
      p.conf_thresh = conf_thresh;
      p.iou_thresh = iou_thresh;
      p.scale = d->scale;
      p.pad_x = d->pad_x;
      p.pad_y = d->pad_y;
      p.orig_w = d->orig_w;
      p.orig_h = d->orig_h;
      p.boxes = d->d_boxes;
      p.cls = d->d_cls;
      p.out = d->d_out;
      p.out_cap = std::min(out_cap, d->max_boxes);
      p.count = d->d_count;
      VP_HIP_CHECK(vp::launch_detect_decode_nms(p, d->stream));
      // count and (at most out_cap) detections come back together: this is the one host synchronisation of a call that has anything to wait for
      VP_HIP_CHECK(hipMemcpyAsync(d->h_count, d->d_count, 2 * sizeof(int), hipMemcpyDeviceToHost, d->stream));
      if (p.out_cap > 0) VP_HIP_CHECK(hipMemcpyAsync(d->h_out, d->d_out, (size_t)p.out_cap * sizeof(vp::Detection), hipMemcpyDeviceToHost, d->stream));
      VP_HIP_CHECK(hipStreamSynchronize(d->stream));   // behind ev_out: the engine's stream has drained too
      g.check_status();
      const int kept = d->h_count[0], n = std::min(kept, p.out_cap);
      if (n > 0) std::memcpy(out, d->h_out, (size_t)n * sizeof(vp::Detection));
      *count = kept;
      return VP_OK;
     } catch (...) {
      // a failure part-way (a launch error, the range probe's verdict): work may still be queued on either stream, and the next call rewrites the
      // engine's input tensor and the staging buffer.  Drain both before the error leaves; the statuses are not looked at, the first error is the news.
      (void)hipStreamSynchronize(g.stream());
      (void)hipStreamSynchronize(d->stream);
      throw;
     }
    } catch (const vp::RangeError& ex) {
      d->err = ex.what();
      return VP_ERR_RANGE;
    }
  });
}

int vp_detect_geometry_pil(int net_h, int net_w, int h, int w, double* scale, int* new_w, int* new_h, int* pad_x, int* pad_y) {
  if (net_h < 1 || net_w < 1 || h < 1 || w < 1 || !scale || !new_w || !new_h || !pad_x || !pad_y) return VP_ERR_ARG;
  return pil_geometry(net_h, net_w, h, w, scale, new_w, new_h, pad_x, pad_y) ? VP_OK : VP_ERR_ARG;
}

int vp_detect_preprocess_pil(vp_detect* d, const uint8_t* frame, int h, int w, int stride_bytes, int pixel_format, float* dst_host_chw) {
  return guarded(d, [&]() -> int {
    letterbox_pil_frame(d, "vp_detect_preprocess_pil", frame, h, w, stride_bytes, pixel_format, d->d_input);
    if (dst_host_chw) VP_HIP_CHECK(hipMemcpyAsync(dst_host_chw, d->d_input, (size_t)3 * d->net_h * d->net_w * sizeof(float), hipMemcpyDeviceToHost, d->stream));
    VP_HIP_CHECK(hipStreamSynchronize(d->stream));
    return VP_OK;
  });
}

int vp_detect_postprocess_agnostic(vp_detect* d, const float* raw, int raw_on_device, int num_attrs, int num_boxes, float conf_thresh, float iou_thresh,
                                   float* out_rows6, int out_cap, int* count) {
  return guarded(d, [&]() -> int {
    if (!raw || !count || out_cap < 0 || (out_cap > 0 && !out_rows6) || num_attrs < 5 || num_attrs > d->max_attrs || num_boxes < 1 || num_boxes > d->max_boxes)
      throw std::invalid_argument("vp_detect_postprocess_agnostic: bad argument (num_attrs / num_boxes within the sizes given to vp_detect_create)");
    if (d->orig_w == 0)
      throw std::invalid_argument("vp_detect_postprocess_agnostic: no letterbox geometry yet (vp_detect_preprocess_pil or vp_detect_set_letterbox first)");
    const float* src = raw;
    if (!raw_on_device) {
      VP_HIP_CHECK(hipMemcpyAsync(d->d_raw, raw, (size_t)num_attrs * num_boxes * sizeof(float), hipMemcpyHostToDevice, d->stream));
      src = d->d_raw;
    }
    const vp::DetectAgnosticParams p = agnostic_params(d, src, num_attrs, num_boxes, conf_thresh, iou_thresh, out_cap);
    VP_HIP_CHECK(vp::launch_detect_agnostic_nms(p, d->stream));
    VP_HIP_CHECK(hipMemcpyAsync(d->h_count, d->d_count, 2 * sizeof(int), hipMemcpyDeviceToHost, d->stream));
    VP_HIP_CHECK(hipStreamSynchronize(d->stream));
    const int kept = d->h_count[0], n = std::min(kept, p.out_cap);
    if (n > 0) {
      VP_HIP_CHECK(hipMemcpyAsync(d->h_out, d->d_out, (size_t)n * 6 * sizeof(float), hipMemcpyDeviceToHost, d->stream));
      VP_HIP_CHECK(hipStreamSynchronize(d->stream));
      std::memcpy(out_rows6, d->h_out, (size_t)n * 6 * sizeof(float));
    }
    *count = kept;
    return VP_OK;
  });
}

int vp_detect_infer_pil(vp_detect* d, const uint8_t* frame, int h, int w, int stride_bytes, int pixel_format, float conf_thresh, float iou_thresh,
                        float* out_rows6, int out_cap, int* count) {
  return guarded(d, [&]() -> int {
    if (!d->net || !d->net->impl) throw std::invalid_argument("vp_detect_infer_pil: no network attached (vp_detect_attach with a VP_AUTOSPEED engine first)");
    if (!count || out_cap < 0 || (out_cap > 0 && !out_rows6)) throw std::invalid_argument("vp_detect_infer_pil: bad output arguments");
    vp::Engine& g = *d->net->impl;
    try {
     try {
      // the event order of vp_detect_infer, stage for stage
      letterbox_pil_frame(d, "vp_detect_infer_pil", frame, h, w, stride_bytes, pixel_format, g.dev_input());
      g.note_device_tensor();
      VP_HIP_CHECK(hipEventRecord(d->ev_in, d->stream));
      VP_HIP_CHECK(hipStreamWaitEvent(g.stream(), d->ev_in, 0));
      g.enqueue();
      g.enqueue_status_fetch();
      VP_HIP_CHECK(hipEventRecord(d->ev_out, g.stream()));
      VP_HIP_CHECK(hipStreamWaitEvent(d->stream, d->ev_out, 0));
      const vp::DetectAgnosticParams p = agnostic_params(d, static_cast<const float*>(g.dev_logits()), g.out_c(), g.out_w(), conf_thresh, iou_thresh, out_cap);
      VP_HIP_CHECK(vp::launch_detect_agnostic_nms(p, d->stream));
      VP_HIP_CHECK(hipMemcpyAsync(d->h_count, d->d_count, 2 * sizeof(int), hipMemcpyDeviceToHost, d->stream));
      if (p.out_cap > 0) VP_HIP_CHECK(hipMemcpyAsync(d->h_out, d->d_out, (size_t)p.out_cap * 6 * sizeof(float), hipMemcpyDeviceToHost, d->stream));
      VP_HIP_CHECK(hipStreamSynchronize(d->stream));
      g.check_status();
      const int kept = d->h_count[0], n = std::min(kept, p.out_cap);
      if (n > 0) std::memcpy(out_rows6, d->h_out, (size_t)n * 6 * sizeof(float));
      *count = kept;
      return VP_OK;
     } catch (...) {
      (void)hipStreamSynchronize(g.stream());   // as vp_detect_infer: both streams drained before the error leaves
      (void)hipStreamSynchronize(d->stream);
      throw;
     }
    } catch (const vp::RangeError& ex) {
      d->err = ex.what();
      return VP_ERR_RANGE;
    }
  });
}

}  // extern "C"

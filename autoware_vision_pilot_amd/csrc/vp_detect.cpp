// vp_detect_*: the AutoSpeed detector's letterbox preprocess and decode + NMS on the device behind the C ABI (include/vp_hip.h; SURVEY.md N4;
// VisionPilot/middleware_recipes/common/backends/autospeed/onnxruntime_engine.cpp:71-113, :170-290).  The detector network is a VP_AUTOSPEED
// engine (engine.cpp build_autospeed) attached with vp_detect_attach: vp_detect_infer runs frame -> detections without leaving the device.  The
// two-call form (a host's own runtime between vp_detect_preprocess and vp_detect_postprocess) stays as it was.
// vp_detect_preprocess_pil / _postprocess_agnostic / _infer_pil: the same three entries in the arithmetic of the Python wrapper
// (Models/inference/auto_speed_infer.py), which letterboxes with Pillow and decodes differently; they share the handle, its buffers and its stored geometry.  Each pair of entries is one
// implementation taking the decode rule (postprocess_rows, infer_rows below; vp::DetectRule, kernels.hpp).
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

namespace {
// an owning buffer of device (hipMalloc) or pinned host (hipHostMalloc) memory, grown on demand: the contents do not survive a growth
template <class T, bool PINNED>
struct Buf {
  T* p = nullptr;
  size_t cap = 0;   // elements
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { release(); }
  void release() {
    if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
  }
  void reserve(size_t n) {
    if (n <= cap) return;
    release();
    VP_HIP_CHECK(PINNED ? hipHostMalloc(reinterpret_cast<void**>(&p), n * sizeof(T)) : hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T)));
    cap = n;
  }
  operator T*() const { return p; }
};
template <class T>
using DevBuf = Buf<T, false>;
template <class T>
using PinBuf = Buf<T, true>;
}  // namespace

struct vp_detect {
  int gpu = 0, net_h = 0, net_w = 0, max_boxes = 0, max_attrs = 0;
  hipStream_t stream = nullptr;
  DevBuf<uint8_t> d_frame;
  PinBuf<uint8_t> h_frame;         // staging
  DevBuf<int> d_xtab, d_ytab;      // [net_w][4], [net_h][4]
  int tab_w = 0, tab_h = 0;
  DevBuf<float> d_input;           // [3][net_h][net_w]
  DevBuf<float> d_raw;             // [max_attrs][max_boxes]
  DevBuf<float> d_boxes;
  DevBuf<int> d_cls;
  DevBuf<vp::Detection> d_out;     // [max_boxes] rows of 24 bytes under either rule (vp::DetectParams::out)
  DevBuf<int> d_count;
  PinBuf<vp::Detection> h_out;     // [max_boxes]
  PinBuf<int> h_count;             // [2]
  // letterbox geometry of the last preprocessed frame (scale_, pad_x_, pad_y_, orig_width_, orig_height_ of the reference engine)
  float scale = 0.0f;
  int pad_x = 0, pad_y = 0, orig_w = 0, orig_h = 0;
  // Pillow letterbox (vp_detect_preprocess_pil): the tables of vp_resample_coeffs for the last frame size, Pillow's u8 image between its two passes,
  // the resized fp32 planes the paste kernel reads
  DevBuf<int> d_pil_tab[4];        // hb, hk, vb, vk
  int pil_hks = 0, pil_vks = 0, pil_w = 0, pil_h = 0;
  DevBuf<uint8_t> d_pil_tmp;
  DevBuf<float> d_pil_planes;      // [3][new_h][new_w], room for [3][net_h][net_w]
  std::string err;
  vp_engine* net = nullptr;        // borrowed VP_AUTOSPEED engine (vp_detect_attach)
  hipEvent_t ev_in = nullptr, ev_out = nullptr;   // input tensor written (detector stream -> engine stream), network done (engine -> detector)

  ~vp_detect() {   // the buffers free themselves behind this body
    (void)hipSetDevice(gpu);
    if (stream) (void)hipStreamSynchronize(stream);
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
    d->d_input.reserve((size_t)3 * net_h * net_w);
    d->d_raw.reserve((size_t)max_attrs * max_boxes);
    d->d_boxes.reserve((size_t)max_boxes * 4);
    d->d_cls.reserve(max_boxes);
    d->d_out.reserve(max_boxes);
    d->d_count.reserve(2);
    d->h_out.reserve(max_boxes);
    d->h_count.reserve(2);
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
void check_frame(const char* who, const uint8_t* frame, int h, int w, int stride_bytes) {
  if (!frame || h < 1 || w < 1 || h > 16384 || w > 16384 || stride_bytes < 3 * w) throw std::invalid_argument(std::string(who) + ": bad frame geometry");
}

void store_geometry(vp_detect* d, float scale, int pad_x, int pad_y, int orig_w, int orig_h) {
  d->scale = scale;
  d->pad_x = pad_x;
  d->pad_y = pad_y;
  d->orig_w = orig_w;
  d->orig_h = orig_h;
}

// the frame's bytes into d->d_frame through the pinned staging buffer, on the detector's stream (both grown on demand)
void upload_frame(vp_detect* d, const uint8_t* bgr, int h, int w, int stride_bytes) {
  const size_t bytes = (size_t)(h - 1) * stride_bytes + (size_t)3 * w;   // a strided view may END with its last pixel: never read a full last stride
  d->d_frame.reserve(bytes);
  d->h_frame.reserve(bytes);
  VP_HIP_CHECK(hipStreamSynchronize(d->stream));  // the staging buffer and the tables must not be rewritten under a copy still in flight (a drained stream: no wait)
  std::memcpy(d->h_frame, bgr, bytes);
  VP_HIP_CHECK(hipMemcpyAsync(d->d_frame, d->h_frame, bytes, hipMemcpyHostToDevice, d->stream));
}

// upload + letterbox of one frame into `dst` ([3][net_h][net_w] fp32) on the detector's stream; no synchronisation behind the launch.  `who`: the
// entry point named in error texts.  Two waits on the detector's own stream, neither of which blocks in steady state: the one ahead of the staging
// copy finds the stream drained (every entry returns synchronised), and the one behind the tap tables runs only when the frame size changes.
// `bring()` puts the frame's bytes into d->d_frame, rows stride_bytes apart, on the detector's stream: the host path's staged upload, or the region copy
// out of a device-resident vp_frame.
template <class Bring>
void letterbox_resident(vp_detect* d, const char* who, Bring&& bring, int h, int w, int stride_bytes, float* dst) {
  // preprocessAutoSpeed :78-98 -- fp32 scale, truncated new size, centred paste
  const float scale = std::min((float)d->net_w / (float)w, (float)d->net_h / (float)h);
  const int new_w = (int)((float)w * scale), new_h = (int)((float)h * scale);
  if (new_w < 1 || new_h < 1 || new_w > d->net_w || new_h > d->net_h) throw std::invalid_argument(std::string(who) + ": the frame collapses under the letterbox scale");
  bring();
  if (d->tab_w != w || d->tab_h != h) {
    std::vector<int> xt, yt;
    vp::linear_taps_u8(w, new_w, &xt);
    vp::linear_taps_u8(h, new_h, &yt);
    d->d_xtab.reserve((size_t)d->net_w * 4);   // new_w <= net_w: room for every frame size
    d->d_ytab.reserve((size_t)d->net_h * 4);
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
  store_geometry(d, scale, p.pad_x, p.pad_y, w, h);
}

void letterbox_frame(vp_detect* d, const char* who, const uint8_t* bgr, int h, int w, int stride_bytes, float* dst) {
  check_frame(who, bgr, h, w, stride_bytes);
  letterbox_resident(d, who, [&] { upload_frame(d, bgr, h, w, stride_bytes); }, h, w, stride_bytes, dst);
}

// the same from a region of a device-resident vp_frame: the detector's stream waits for the frame's content, copies the region device to device (rows
// packed) and tells the frame that a consumer's copy is queued; the letterbox launch behind it is the host path's
void letterbox_from_frame(vp_detect* d, const char* who, vp_frame* f, int x0, int y0, int w, int h, float* dst) {
  const vp::FrameView v = f->view();
  if (v.gpu != d->gpu) throw std::invalid_argument(std::string(who) + ": the frame lives on GPU " + std::to_string(v.gpu) + ", the detector on GPU " + std::to_string(d->gpu));
  vp::resolve_frame_region(v, x0, y0, &w, &h);
  letterbox_resident(d, who, [&] {
    d->d_frame.reserve((size_t)h * 3 * w);   // a growth frees the old buffer: every entry returns with the stream drained, nothing reads it
    VP_HIP_CHECK(hipStreamWaitEvent(d->stream, v.ready, 0));
    VP_HIP_CHECK(hipMemcpy2DAsync(d->d_frame, (size_t)3 * w, v.bgr + (size_t)y0 * v.pitch + (size_t)3 * x0, v.pitch, (size_t)3 * w, h, hipMemcpyDeviceToDevice, d->stream));
    f->note_consumer(d->stream);
  }, h, w, 3 * w, dst);
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
  check_frame(who, frame, h, w, stride_bytes);
  if (pixel_format != VP_BGR8 && pixel_format != VP_RGB8) throw std::invalid_argument(std::string(who) + ": pixel_format is VP_BGR8 or VP_RGB8");
  double scale = 0.0;
  int new_w = 0, new_h = 0, pad_x = 0, pad_y = 0;
  if (!pil_geometry(d->net_h, d->net_w, h, w, &scale, &new_w, &new_h, &pad_x, &pad_y))
    throw std::invalid_argument(std::string(who) + ": the frame collapses under the letterbox scale");
  upload_frame(d, frame, h, w, stride_bytes);
  d->d_pil_planes.reserve((size_t)3 * d->net_h * d->net_w);
  if (d->pil_w != w || d->pil_h != h) {
    std::vector<int> tab[4];
    const int hks = vp::pil_coeffs(w, new_w, 1, &tab[0], &tab[1]), vks = vp::pil_coeffs(h, new_h, 1, &tab[2], &tab[3]);
    d->pil_w = d->pil_h = 0;
    for (int i = 0; i < 4; ++i) {   // once per frame size: the tap count follows the size
      d->d_pil_tab[i].reserve(tab[i].size());
      VP_HIP_CHECK(hipMemcpyAsync(d->d_pil_tab[i], tab[i].data(), tab[i].size() * sizeof(int), hipMemcpyHostToDevice, d->stream));
    }
    d->d_pil_tmp.reserve((size_t)h * new_w * 3);
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
  store_geometry(d, (float)scale, pad_x, pad_y, w, h);
}

// the decode + NMS launch on the detector's stream: `raw` on the device, the handle's scratch, rows and counts, its stored geometry
vp::DetectParams launch_decode(vp_detect* d, vp::DetectRule rule, const float* raw, int num_attrs, int num_boxes, float conf_thresh, float iou_thresh, int out_cap) {
  vp::DetectParams p{};
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
  p.out = d->d_out;
  p.out_cap = std::min(out_cap, d->max_boxes);
  p.count = d->d_count;
  VP_HIP_CHECK(vp::launch_detect_nms(p, rule, d->stream));
  return p;
}

constexpr size_t kRow = sizeof(vp::Detection);   // 24 bytes under either rule: a vp_detection, or six floats

// vp_detect_postprocess / _postprocess_agnostic: raw tensor in, rows out.  The count comes back first, then exactly the rows there are.
int postprocess_rows(vp_detect* d, vp::DetectRule rule, const float* raw, int raw_on_device, int num_attrs, int num_boxes, float conf_thresh, float iou_thresh,
                     void* out, int out_cap, int* count) {
  const bool agnostic = rule == vp::kDetectAgnostic;
  const char* who = agnostic ? "vp_detect_postprocess_agnostic" : "vp_detect_postprocess";
  return guarded(d, [&]() -> int {
    if (!raw || !count || out_cap < 0 || (out_cap > 0 && !out) || num_attrs < 5 || num_attrs > d->max_attrs || num_boxes < 1 || num_boxes > d->max_boxes)
      throw std::invalid_argument(std::string(who) + ": bad argument (num_attrs / num_boxes within the sizes given to vp_detect_create)");
    if (d->orig_w == 0)
      throw std::invalid_argument(std::string(who) + ": no letterbox geometry yet (" + (agnostic ? "vp_detect_preprocess_pil" : "vp_detect_preprocess") + " or vp_detect_set_letterbox first)");
    const float* src = raw;
    if (!raw_on_device) {
      VP_HIP_CHECK(hipMemcpyAsync(d->d_raw, raw, (size_t)num_attrs * num_boxes * sizeof(float), hipMemcpyHostToDevice, d->stream));
      src = d->d_raw;
    }
    const vp::DetectParams p = launch_decode(d, rule, src, num_attrs, num_boxes, conf_thresh, iou_thresh, out_cap);
    VP_HIP_CHECK(hipMemcpyAsync(d->h_count, d->d_count, 2 * sizeof(int), hipMemcpyDeviceToHost, d->stream));
    VP_HIP_CHECK(hipStreamSynchronize(d->stream));
    const int kept = d->h_count[0], n = std::min(kept, p.out_cap);
    if (n > 0) {
      VP_HIP_CHECK(hipMemcpyAsync(d->h_out, d->d_out, (size_t)n * kRow, hipMemcpyDeviceToHost, d->stream));
      VP_HIP_CHECK(hipStreamSynchronize(d->stream));
      std::memcpy(out, d->h_out, (size_t)n * kRow);
    }
    *count = kept;
    return VP_OK;
  });
}

// vp_detect_infer / _infer_pil: frame in, rows out through the attached engine without leaving the device.  `letterbox(who, dst)` uploads the frame
// and writes the network's input tensor on the detector's stream.
template <class Letterbox>
int infer_rows(vp_detect* d, vp::DetectRule rule, Letterbox&& letterbox, float conf_thresh, float iou_thresh, void* out, int out_cap, int* count) {
  const char* who = rule == vp::kDetectAgnostic ? "vp_detect_infer_pil" : "vp_detect_infer";
  return guarded(d, [&]() -> int {
    if (!d->net || !d->net->impl) throw std::invalid_argument(std::string(who) + ": no network attached (vp_detect_attach with a VP_AUTOSPEED engine first)");
    if (!count || out_cap < 0 || (out_cap > 0 && !out)) throw std::invalid_argument(std::string(who) + ": bad output arguments");
    vp::Engine& g = *d->net->impl;
    try {
     try {
      // letterbox straight into the network's input tensor: every exit of this call, the failing ones included (see the handler below), leaves both
      // streams drained, so nothing still reads it
      letterbox(who, g.dev_input());
      g.note_device_tensor();
      VP_HIP_CHECK(hipEventRecord(d->ev_in, d->stream));
      VP_HIP_CHECK(hipStreamWaitEvent(g.stream(), d->ev_in, 0));
      g.enqueue();         // the replayed graph (first call: the eager warm-up pass)
      g.enqueue_status_fetch();   // the range probe's verdict behind it; the output tensor itself stays on the device
      VP_HIP_CHECK(hipEventRecord(d->ev_out, g.stream()));
      VP_HIP_CHECK(hipStreamWaitEvent(d->stream, d->ev_out, 0));
      const vp::DetectParams p = launch_decode(d, rule, static_cast<const float*>(g.dev_logits()), g.out_c(), g.out_w(), conf_thresh, iou_thresh, out_cap);
      // count and (at most out_cap) detections come back together: this is the one host synchronisation of a call that has anything to wait for
      VP_HIP_CHECK(hipMemcpyAsync(d->h_count, d->d_count, 2 * sizeof(int), hipMemcpyDeviceToHost, d->stream));
      if (p.out_cap > 0) VP_HIP_CHECK(hipMemcpyAsync(d->h_out, d->d_out, (size_t)p.out_cap * kRow, hipMemcpyDeviceToHost, d->stream));
      VP_HIP_CHECK(hipStreamSynchronize(d->stream));   // behind ev_out: the engine's stream has drained too
      g.check_status();
      const int kept = d->h_count[0], n = std::min(kept, p.out_cap);
      if (n > 0) std::memcpy(out, d->h_out, (size_t)n * kRow);
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
  store_geometry(d, scale, pad_x, pad_y, orig_w, orig_h);
  return VP_OK;
}

int vp_detect_postprocess(vp_detect* d, const float* raw, int raw_on_device, int num_attrs, int num_boxes, float conf_thresh, float iou_thresh,
                          vp_detection* out, int out_cap, int* count) {
  return postprocess_rows(d, vp::kDetectPerClass, raw, raw_on_device, num_attrs, num_boxes, conf_thresh, iou_thresh, out, out_cap, count);
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
  return infer_rows(d, vp::kDetectPerClass, [&](const char* who, float* dst) { letterbox_frame(d, who, bgr, h, w, stride_bytes, dst); }, conf_thresh, iou_thresh, out, out_cap,
                    count);
}

int vp_detect_infer_frame(vp_detect* d, vp_frame* f, int x0, int y0, int w, int h, float conf_thresh, float iou_thresh, vp_detection* out, int out_cap,
                          int* count) {
  if (!d) return VP_ERR_ARG;
  if (!f) {
    d->err = "vp_detect_infer_frame: null frame";
    return VP_ERR_ARG;
  }
  if (!f->uploaded) {
    d->err = "vp_detect_infer_frame: the frame was never uploaded (vp_frame_upload / vp_frame_upload_device first)";
    return VP_ERR_STATE;
  }
  return infer_rows(d, vp::kDetectPerClass, [&](const char*, float* dst) { letterbox_from_frame(d, "vp_detect_infer_frame", f, x0, y0, w, h, dst); }, conf_thresh,
                    iou_thresh, out, out_cap, count);
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
  return postprocess_rows(d, vp::kDetectAgnostic, raw, raw_on_device, num_attrs, num_boxes, conf_thresh, iou_thresh, out_rows6, out_cap, count);
}

int vp_detect_infer_pil(vp_detect* d, const uint8_t* frame, int h, int w, int stride_bytes, int pixel_format, float conf_thresh, float iou_thresh,
                        float* out_rows6, int out_cap, int* count) {
  return infer_rows(d, vp::kDetectAgnostic, [&](const char* who, float* dst) { letterbox_pil_frame(d, who, frame, h, w, stride_bytes, pixel_format, dst); }, conf_thresh,
                    iou_thresh, out_rows6, out_cap, count);
}

}  // extern "C"

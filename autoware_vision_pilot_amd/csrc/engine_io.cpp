// libvp_hip engine, part 3 of 3: the per-frame path around the plan -- input format and resize tables, frame upload, eager run / hipGraph
// capture and replay (single engine and base + shared heads), output fetch and the range probe's verdict, resizes, visualisation, timers.
#include "engine_internal.hpp"

#include <climits>
#include <cstdint>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/vp_hip.h"

namespace vp {

// ------------------------------------------------------------------------------------------ frame handling
void Engine::set_input_format(int pixel_format, int plane_order) {
  if (pixel_format < 0 || pixel_format > 1 || plane_order < 0 || plane_order > 1) throw std::invalid_argument("bad input format");
  if (pixel_format != pixel_format_ || plane_order != plane_order_) { graph_valid_ = false; ++plan_epoch_; }
  pixel_format_ = pixel_format;
  plane_order_ = plane_order;
}
void Engine::set_norm_form(int form) {
  if (form < 0 || form > 1) throw std::invalid_argument("norm form: 0 = q / 255 (torchvision to_tensor), 1 = q * fl(1/255) (cv::Mat::convertTo)");
  if (base_) throw std::invalid_argument("shared engine: the base engine owns the frame path");
  if (form != norm_form_) { graph_valid_ = false; ++plan_epoch_; }
  norm_form_ = form;
}
void Engine::set_lane_ring(bool on) {
  if (kind_ != 3) throw std::invalid_argument("lane ring: VP_EGOLANES engines only (the AutoSteer hand-over of the EgoLanes logits)");
  if (on == lane_ring_) return;
  VP_HIP_CHECK(hipSetDevice(gpu_));
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
  if (on && !d_lane_ring_) d_lane_ring_ = static_cast<float*>(dalloc((size_t)2 * out_c_ * out_h_ * out_w_ * sizeof(float), true));
  if (on) fill_zero(d_lane_ring_, (size_t)2 * out_c_ * out_h_ * out_w_ * sizeof(float));
  lane_ring_ = on;
  ring_frames_ = 0;
  graph_valid_ = false;
  ++plan_epoch_;
}
void Engine::fetch_lane_ring(float* dst) {
  if (!lane_ring_ || !d_lane_ring_) throw std::runtime_error("lane ring is not enabled (vp_set_lane_ring)");
  if (!dst) throw std::invalid_argument("null destination");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  VP_HIP_CHECK(hipMemcpyAsync(dst, d_lane_ring_, (size_t)2 * out_c_ * out_h_ * out_w_ * sizeof(float), hipMemcpyDeviceToHost, stream_));
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
}
void Engine::set_decode_mode(int mode) {
  if (mode < 0 || mode > 2) throw std::invalid_argument("bad decode mode");
  if (mode != decode_mode_) { graph_valid_ = false; ++plan_epoch_; }
  decode_mode_ = mode;
}

// 11-bit fixed-point bilinear taps -- must stay bit-identical to oracle/pre_post.py linear_taps_u8.
void linear_taps_u8(int src, int dst, std::vector<int>* tab) {
  tab->resize((size_t)dst * 4);
  const double scale = (double)src / (double)dst;
  for (int d = 0; d < dst; ++d) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)std::floor(f);
    f -= (float)s;
    if (s < 0) {
      f = 0.0f;
      s = 0;
    }
    if (s >= src - 1) {
      f = 0.0f;
      s = src - 1;
    }
    (*tab)[4 * d + 0] = s;
    (*tab)[4 * d + 1] = std::min(s + 1, src - 1);
    (*tab)[4 * d + 2] = (int)std::nearbyint((1.0f - f) * 2048.0f);
    (*tab)[4 * d + 3] = (int)std::nearbyint(f * 2048.0f);
  }
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc (src/libImaging/Resample.c) in the same double arithmetic, operation for
// operation (restated and pinned against PIL in oracle/pre_post.py pil_resample_coeffs): filter support scaled by the
// down-scaling factor, taps normalised to sum 1, quantised to 22 fractional bits.  filter: 1 = BILINEAR, 2 = BICUBIC (a = -0.5).
#pragma clang fp contract(off)
int pil_coeffs(int in_size, int out_size, int filter, std::vector<int>* bounds, std::vector<int>* kk) {
  auto weight = [filter](double x) -> double {
    if (x < 0.0) x = -x;
    if (filter == 1) return x < 1.0 ? 1.0 - x : 0.0;
    const double a = -0.5;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
  };
  double filterscale = (double)in_size / out_size;
  const double scale = filterscale;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = (filter == 1 ? 1.0 : 2.0) * filterscale;
  const int ksize = (int)std::ceil(support) * 2 + 1;
  bounds->assign((size_t)out_size * 2, 0);
  kk->assign((size_t)out_size * ksize, 0);
  std::vector<double> k(ksize);
  const double ss = 1.0 / filterscale;
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    double ww = 0.0;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    for (int x = 0; x < xmax; ++x) {
      const double w = weight((x + xmin - center + 0.5) * ss);
      k[x] = w;
      ww += w;
    }
    for (int x = 0; x < xmax; ++x) {
      if (ww != 0.0) k[x] /= ww;
      (*kk)[(size_t)xx * ksize + x] = k[x] < 0 ? (int)(-0.5 + k[x] * (1 << 22)) : (int)(0.5 + k[x] * (1 << 22));
    }
    (*bounds)[2 * xx] = xmin;
    (*bounds)[2 * xx + 1] = xmax;
  }
  return ksize;
}

PilResampleParams Engine::pil_params(const PreprocessParams& pp) const {
  PilResampleParams q{};
  q.frame = pp.frame;
  q.stride = pp.stride;
  q.in_h = frame_h_;
  q.in_w = frame_w_;
  q.out_h = pp.out_h;
  q.out_w = pp.out_w;
  q.hb = d_pil_hb_;
  q.hk = d_pil_hk_;
  q.hks = pil_hks_;
  q.vb = d_pil_vb_;
  q.vk = d_pil_vk_;
  q.vks = pil_vks_;
  q.tmp = d_pil_tmp_;
  for (int c = 0; c < 3; ++c) {
    q.src_c[c] = pp.src_c[c];
    q.mean[c] = pp.mean[c];
    q.stdv[c] = pp.stdv[c];
  }
  q.out = pp.out;
  q.norm_form = pp.norm_form;
  return q;
}

void Engine::set_resize_mode(int mode) {
  if (mode < 0 || mode > 2) throw std::invalid_argument("resize mode: 0 = cv::resize INTER_LINEAR model, 1 = PIL BILINEAR, 2 = PIL BICUBIC");
  if (base_) throw std::invalid_argument("shared engine: the base engine owns the frame path");
  if (kind_ == 6 && mode != 0) throw std::invalid_argument("VP_AUTOSTEER: the network takes the 512 x 1024 frame as it is (no resize)");
  if (mode != resize_mode_) {
    resize_mode_ = mode;
    tab_h_ = tab_w_ = 0;
    graph_valid_ = false;
    ++plan_epoch_;
  }
}

void Engine::ensure_tables(int h, int w) {
  if (h == tab_h_ && w == tab_w_) return;
  if (resize_mode_ != 0) {  // Pillow's resample: per-output tap tables for both passes + the u8 image between them
    std::vector<int> hb, hk, vb, vk;
    pil_hks_ = pil_coeffs(w, net_w(), resize_mode_, &hb, &hk);
    pil_vks_ = pil_coeffs(h, net_h(), resize_mode_, &vb, &vk);
    VP_HIP_CHECK(hipStreamSynchronize(stream_));
    // capacity-tracked: a host alternating between frame geometries re-uses (or re-grows and FREES) these five buffers instead of
    // leaking a set per change
    upload_grow(d_pil_hb_, pil_cap_[0], hb);
    upload_grow(d_pil_hk_, pil_cap_[1], hk);
    upload_grow(d_pil_vb_, pil_cap_[2], vb);
    upload_grow(d_pil_vk_, pil_cap_[3], vk);
    const size_t tmp_need = (size_t)h * net_w() * 3;
    if (tmp_need > pil_cap_[4]) {
      dfree(d_pil_tmp_);
      d_pil_tmp_ = static_cast<uint8_t*>(dalloc(tmp_need, false));
      pil_cap_[4] = tmp_need;
    }
    tab_h_ = h;
    tab_w_ = w;
    return;
  }
  std::vector<int> xt, yt;
  linear_taps_u8(w, net_w(), &xt);
  linear_taps_u8(h, net_h(), &yt);
  if (!d_xtab_) {
    d_xtab_ = static_cast<int*>(dalloc(net_w() * 4 * sizeof(int)));
    d_ytab_ = static_cast<int*>(dalloc(net_h() * 4 * sizeof(int)));
  }
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
  copy_h2d(d_xtab_, xt.data(), xt.size() * sizeof(int));
  copy_h2d(d_ytab_, yt.data(), yt.size() * sizeof(int));
  tab_h_ = h;
  tab_w_ = w;
}

// ---- frame pools registered for DMA (vp_register_frames): a short sorted table behind a mutex; the lookup is two compares per range
namespace {
std::mutex g_pool_mu;
std::vector<std::pair<uintptr_t, size_t>> g_pools;   // [begin, bytes), disjoint
}  // namespace
int register_frame_range(const void* pool, size_t bytes) {
  if (!pool || bytes == 0) return VP_ERR_ARG;
  const uintptr_t b = reinterpret_cast<uintptr_t>(pool);
  std::lock_guard<std::mutex> lk(g_pool_mu);
  for (const auto& r : g_pools)
    if (b < r.first + r.second && r.first < b + bytes) return VP_ERR_ARG;   // overlaps a registered range
  if (hipHostRegister(const_cast<void*>(pool), bytes, hipHostRegisterPortable) != hipSuccess) {
    (void)hipGetLastError();
    return VP_ERR_HIP;
  }
  g_pools.emplace_back(b, bytes);
  return VP_OK;
}
int unregister_frame_range(const void* pool) {
  if (!pool) return VP_ERR_ARG;
  const uintptr_t b = reinterpret_cast<uintptr_t>(pool);
  std::lock_guard<std::mutex> lk(g_pool_mu);
  for (size_t i = 0; i < g_pools.size(); ++i)
    if (g_pools[i].first == b) {
      // unlock first, forget only on success: a refused unlock (a DMA still in flight) leaves the range page-locked AND tracked, so frames from it keep
      // the one-DMA path and a later retry finds it (erased first, a failure left it locked but unknown)
      if (hipHostUnregister(const_cast<void*>(pool)) != hipSuccess) {
        (void)hipGetLastError();
        return VP_ERR_HIP;
      }
      g_pools.erase(g_pools.begin() + i);
      return VP_OK;
    }
  return VP_ERR_ARG;
}
bool frame_range_registered(const void* p, size_t bytes) {
  const uintptr_t b = reinterpret_cast<uintptr_t>(p);
  std::lock_guard<std::mutex> lk(g_pool_mu);
  for (const auto& r : g_pools)
    if (b >= r.first && b + bytes <= r.first + r.second) return true;
  return false;
}

void Engine::refuse_frame_input() const {
  if (base_) throw std::invalid_argument("shared engine: frames go to the base engine (vp_infer on the base, then vp_infer_shared)");
  if (kind_ == 5) throw std::runtime_error("VP_AUTOSPEED engines have no frame preprocess of their own: attach the engine to a detector (vp_detect_attach) and call vp_detect_infer, or hand the letterboxed tensor to vp_infer_tensor");
}

// First half of every frame upload (host bytes: upload_frame; a device-resident vp_frame: upload_from_frame): the refusals, the frame buffer, the tap
// tables and the graph invalidation a new geometry brings.  Returns where slot `index`'s bytes go.
uint8_t* Engine::accept_frame_geometry(bool have_bytes, int h, int w, int stride, int index) {
  refuse_frame_input();
  if (!have_bytes || h < 2 || w < 2 || stride < 3 * w) throw std::invalid_argument("bad frame geometry");
  if (kind_ == 6 && (h != net_h() || w != net_w()))   // auto_steer_infer.py:37-39 raises ValueError: this network has no resize in front of it
    throw std::invalid_argument("VP_AUTOSTEER: the input frame must be 512 x 1024 (height x width), got " + std::to_string(h) + " x " + std::to_string(w));
  if (index < 0 || index >= frames_) throw std::invalid_argument("frame index out of range");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  prev_frame_valid_ = prev_frame_stashed_;   // VP_ACT_SCALE: a stashed previous frame belongs to the upload right behind it only
  prev_frame_stashed_ = false;
  const size_t need = (size_t)h * stride;
  if ((h != frame_h_ || w != frame_w_ || stride != frame_stride_) && frames_ > 1 && index != 0 && frame_h_ != 0)
    throw std::invalid_argument("batched encoder: all frames of a pass share one geometry (upload slot 0 first to change it)");
  if (need * frames_ > frame_cap_) {
    VP_HIP_CHECK(hipStreamSynchronize(stream_));
    dfree(d_frame_);
    d_frame_ = static_cast<uint8_t*>(dalloc(need * frames_, true));
    frame_cap_ = need * frames_;
    { graph_valid_ = false; ++plan_epoch_; }
  }
  if (h != frame_h_ || w != frame_w_ || stride != frame_stride_) { graph_valid_ = false; ++plan_epoch_; }
  ensure_tables(h, w);
  frame_h_ = h;
  frame_w_ = w;
  frame_stride_ = stride;
  return d_frame_ + (size_t)index * need;
}

void Engine::note_frame_input() {
  if (input_is_tensor_) { graph_valid_ = false; ++plan_epoch_; }
  input_is_tensor_ = false;
}

void resolve_frame_region(const FrameView& f, int x0, int y0, int* w, int* h) {
  if (!f.bgr) throw std::runtime_error("the frame was never uploaded (vp_frame_upload / vp_frame_upload_device first)");
  if (*w == 0 && *h == 0 && x0 == 0 && y0 == 0) {
    *w = f.w;
    *h = f.h;
  }
  if (x0 < 0 || y0 < 0 || *w < 2 || *h < 2 || (long long)x0 + *w > f.w || (long long)y0 + *h > f.h)
    throw std::invalid_argument("frame region (x0 " + std::to_string(x0) + ", y0 " + std::to_string(y0) + ", " + std::to_string(*w) + " x " + std::to_string(*h) +
                                ") must be at least 2 x 2 and lie inside the " + std::to_string(f.w) + " x " + std::to_string(f.h) + " frame");
}

void Engine::upload_from_frame(const FrameView& f, int x0, int y0, int w, int h) {
  refuse_frame_input();
  if (frames_ > 1) throw std::invalid_argument("batched encoder: frames from a vp_frame are not supported (vp_upload_frame_n takes host frames)");
  if (pixel_format_ != 0) throw std::invalid_argument("vp_frame holds BGR8: the engine's input pixel format must be VP_BGR8 (vp_set_input_format)");
  if (f.gpu != gpu_) throw std::invalid_argument("the frame lives on GPU " + std::to_string(f.gpu) + ", the engine on GPU " + std::to_string(gpu_));
  resolve_frame_region(f, x0, y0, &w, &h);
  uint8_t* dst = accept_frame_geometry(true, h, w, 3 * w, 0);
  VP_HIP_CHECK(hipStreamWaitEvent(stream_, f.ready, 0));   // never a host wait: the copy runs once the frame's content is complete
  VP_HIP_CHECK(hipMemcpy2DAsync(dst, (size_t)3 * w, f.bgr + (size_t)y0 * f.pitch + (size_t)3 * x0, f.pitch, (size_t)3 * w, h, hipMemcpyDeviceToDevice, stream_));
  src_region_ = {x0, y0, w, h, f.h, f.w};
  note_frame_input();
}

void Engine::upload_frame(const uint8_t* frame, int h, int w, int stride, int index) {
  uint8_t* dst = accept_frame_geometry(frame != nullptr, h, w, stride, index);
  const size_t need = (size_t)h * stride;
  // A strided view (cv::Mat ROI, numpy slice) guarantees only (h-1)*stride + 3*w readable bytes: the tail of the last row
  // belongs to the parent image or to nobody.  Packed frames go as one copy, views row by row (hipMemcpy2D).
  // The caller's buffer is pageable (cv::Mat); the copy is staged through this engine's pinned buffer so the transfer
  // itself is one DMA that overlaps other engines' kernels (the reference does the same H2D: tensorrt_backend.cpp:184-186).
  const size_t packed = (size_t)(h - 1) * stride + (size_t)3 * w;
  // a frame inside a pool the host registered (vp_register_frames) is page-locked already: one DMA straight from the caller's memory
  const bool staged = pinned_staging_ && !frame_range_registered(frame, packed);
  if (staged) {
    if (need > h_frame_cap_) {
      VP_HIP_CHECK(hipStreamSynchronize(stream_));
      if (h_frame_) hipHostFree(h_frame_);
      h_frame_ = nullptr;
      VP_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&h_frame_), need * 2, hipHostMallocDefault));  // two slots: frame n+1 is staged while n flies
      h_frame_cap_ = need;
    }
    h_frame_slot_ ^= 1;
    uint8_t* slot = h_frame_ + (size_t)h_frame_slot_ * h_frame_cap_;
    // A pinned source makes the H2D below truly asynchronous: the copy that last read this slot (two uploads ago) may still be
    // queued behind earlier frames' graphs.  Its event orders this host write behind it.
    if (!h_frame_ev_[h_frame_slot_]) VP_HIP_CHECK(hipEventCreateWithFlags(&h_frame_ev_[h_frame_slot_], hipEventDisableTiming));
    else VP_HIP_CHECK(hipEventSynchronize(h_frame_ev_[h_frame_slot_]));
    if (stride == 3 * w) {
      std::memcpy(slot, frame, packed);
    } else {
      for (int y = 0; y < h; ++y) std::memcpy(slot + (size_t)y * stride, frame + (size_t)y * stride, (size_t)3 * w);
    }
    VP_HIP_CHECK(hipMemcpyAsync(dst, slot, packed, hipMemcpyHostToDevice, stream_));
    VP_HIP_CHECK(hipEventRecord(h_frame_ev_[h_frame_slot_], stream_));
  } else if (stride == 3 * w) {
    VP_HIP_CHECK(hipMemcpyAsync(dst, frame, packed, hipMemcpyHostToDevice, stream_));
  } else {
    VP_HIP_CHECK(hipMemcpy2DAsync(dst, stride, frame, stride, (size_t)3 * w, h, hipMemcpyHostToDevice, stream_));
  }
  src_region_ = {0, 0, w, h, h, w};   // a host frame is its own source
  note_frame_input();
}

void Engine::upload_tensor(const float* nchw) {
  if (base_) throw std::invalid_argument("shared engine: tensors go to the base engine");
  if (frames_ > 1) throw std::invalid_argument("batched encoder: frames only (vp_upload_frame_n)");
  if (!nchw) throw std::invalid_argument("null tensor");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  VP_HIP_CHECK(hipMemcpyAsync(d_input_, nchw, (size_t)3 * net_h() * net_w() * sizeof(float), hipMemcpyHostToDevice, stream_));
  if (!input_is_tensor_) { graph_valid_ = false; ++plan_epoch_; }
  input_is_tensor_ = true;
}

void Engine::note_device_tensor() {
  if (kind_ != 5) throw std::invalid_argument("note_device_tensor: VP_AUTOSPEED engines only");
  if (!input_is_tensor_) { graph_valid_ = false; ++plan_epoch_; }
  input_is_tensor_ = true;
}

void Engine::run_ops(hipStream_t st, size_t begin, size_t end) {
  for (size_t i = begin; i < end; ++i) {
    hipError_t e = ops_[i].run(st);
    if (e != hipSuccess) throw std::runtime_error("launch failed in layer '" + ops_[i].name + "': " + hipGetErrorString(e));
  }
}
void Engine::run_eager() { run_ops(stream_, input_is_tensor_ ? first_net_op_ : 0, ops_.size()); }

// One frame through this engine AND its shared-prefix heads as ONE graph launch on this engine's stream (so every stream-order
// guarantee of the separate vp_enqueue calls holds).  Inside the graph the heads that consume only the backbone (shared level 1:
// Scene3D, EgoLanes on a SceneSeg base) are forked onto side streams right behind the backbone and joined at the end: a single
// frame's two or three decoders overlap (the small-map neck layers and the 200-tile big layers leave CUs idle on their own).
// Same kernels, same arguments, same results as base.enqueue() followed by head.enqueue().
void Engine::enqueue_multi(const std::vector<Engine*>& heads) {
  VP_HIP_CHECK(hipSetDevice(gpu_));
  if (base_) throw std::invalid_argument("enqueue_multi: call it on the engine that owns the encoder");
  for (Engine* h : heads)
    if (!h || h->base_ != this || h->stream_ != stream_) throw std::invalid_argument("enqueue_multi: every head must be a shared-prefix engine of this engine");
  bool plain = !multi_fork_ || !use_graph_ || !warmed_ || kind_ == 4 || frames_ > 1 || n_fork_ops_ == 0 || heads.empty();
  for (Engine* h : heads) plain = plain || !h->warmed_ || !h->use_graph_;
  if (plain) {  // first frames (eager warm-up), graph replay switched off, or nothing to fork
    enqueue();
    for (Engine* h : heads) h->enqueue();
    return;
  }
  if (!input_is_tensor_ && !d_frame_) throw std::runtime_error("no frame resident: call vp_upload_frame / vp_infer first");
  std::vector<std::pair<const Engine*, unsigned long long>> key{{this, plan_epoch_}};
  for (Engine* h : heads) key.emplace_back(h, h->plan_epoch_);
  if (!multi_exec_ || key != multi_key_) {
    if (multi_exec_) hipGraphExecDestroy(multi_exec_);
    if (multi_graph_) hipGraphDestroy(multi_graph_);
    multi_exec_ = nullptr;
    multi_graph_ = nullptr;
    size_t n_side = 0;
    for (Engine* h : heads) n_side += h->shared_level_ == 1 ? 1 : 0;
    while (side_streams_.size() < n_side) {
      hipStream_t s = nullptr;
      VP_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      side_streams_.push_back(s);
    }
    while (side_events_.size() < n_side + 1) {
      hipEvent_t e = nullptr;
      VP_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      side_events_.push_back(e);
    }
    VP_HIP_CHECK(hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal));
    try {
      const size_t first = input_is_tensor_ ? first_net_op_ : 0;
      run_ops(stream_, first, n_fork_ops_);
      VP_HIP_CHECK(hipEventRecord(side_events_[0], stream_));
      size_t si = 0;
      for (Engine* h : heads)
        if (h->shared_level_ == 1) {
          VP_HIP_CHECK(hipStreamWaitEvent(side_streams_[si], side_events_[0], 0));
          h->run_ops(side_streams_[si], 0, h->ops_.size());
          VP_HIP_CHECK(hipEventRecord(side_events_[1 + si], side_streams_[si]));
          ++si;
        }
      run_ops(stream_, n_fork_ops_, ops_.size());
      for (Engine* h : heads)
        if (h->shared_level_ != 1) h->run_ops(stream_, 0, h->ops_.size());  // needs this engine's context + neck: behind them, in order
      for (size_t i = 0; i < si; ++i) VP_HIP_CHECK(hipStreamWaitEvent(stream_, side_events_[1 + i], 0));
    } catch (...) {
      hipGraph_t g = nullptr;
      hipStreamEndCapture(stream_, &g);
      if (g) hipGraphDestroy(g);
      throw;
    }
    VP_HIP_CHECK(hipStreamEndCapture(stream_, &multi_graph_));
    VP_HIP_CHECK(hipGraphInstantiate(&multi_exec_, multi_graph_, nullptr, nullptr, 0));
    multi_key_ = key;
  }
  VP_HIP_CHECK(hipGraphLaunch(multi_exec_, stream_));
  have_outputs_ = true;
  host_logits_valid_ = host_mask_valid_ = false;
  note_pass();
  for (Engine* h : heads) {
    h->have_outputs_ = true;
    h->host_logits_valid_ = h->host_mask_valid_ = false;
    h->note_pass();
  }
}

void Engine::capture_graph() {
  if (graph_exec_) {
    hipGraphExecDestroy(graph_exec_);
    graph_exec_ = nullptr;
  }
  if (graph_) {
    hipGraphDestroy(graph_);
    graph_ = nullptr;
  }
  VP_HIP_CHECK(hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal));
  try {
    run_eager();
  } catch (...) {
    hipGraph_t g = nullptr;
    hipStreamEndCapture(stream_, &g);
    if (g) hipGraphDestroy(g);
    throw;
  }
  VP_HIP_CHECK(hipStreamEndCapture(stream_, &graph_));
  VP_HIP_CHECK(hipGraphInstantiate(&graph_exec_, graph_, nullptr, nullptr, 0));
  graph_valid_ = true;
}

void Engine::enqueue() {
  VP_HIP_CHECK(hipSetDevice(gpu_));
  if (base_) {
    if (!base_->have_outputs_) throw std::runtime_error("shared engine: run the base engine on a frame first");
  } else if (!input_is_tensor_ && !d_frame_) {
    throw std::runtime_error("no frame resident: call vp_upload_frame / vp_infer first");
  }
  if (kind_ == 4 && !ad_primed_) prime_previous();  // first frame of a stream: previous := current
  if (!warmed_) {  // first pass is eager: sets kernel attributes and surfaces launch errors with layer names
    run_eager();
    VP_HIP_CHECK(hipStreamSynchronize(stream_));
    warmed_ = true;
    have_outputs_ = true;
    host_logits_valid_ = host_mask_valid_ = false;
    if (!use_graph_ || kind_ == 4 || lane_ring_) {  // AutoDrive (feature shift) and the lane ring carry state: a frame must run exactly once
      note_pass();
      return;
    }
  }
  if (use_graph_) {
    if (!graph_valid_) capture_graph();
    VP_HIP_CHECK(hipGraphLaunch(graph_exec_, stream_));
  } else {
    run_eager();
  }
  have_outputs_ = true;
  host_logits_valid_ = host_mask_valid_ = false;
  note_pass();
}

void Engine::sync() {
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
  check_status();
}

// The probe's verdict on the pass whose outputs were last fetched (enqueue_fetch copies the flag behind them).  The flag is PER PASS: the
// probe kernel overwrites every word of it on every pass (kernels_misc.hip; nothing to clear, nothing sticky), so a bad frame is reported once, by the call that fetches THAT frame, and a
// pass that was enqueued but never fetched leaves nothing behind for a later frame.
bool Engine::poll_status() {
  if (!status_pending_ || !h_status_) return false;
  status_pending_ = false;
  unsigned bad = 0;
  for (int i = 0; i < VP_PROBE_BLOCKS; ++i) bad |= h_status_[i];
  std::memset(h_status_, 0, VP_PROBE_BLOCKS * sizeof(unsigned));
  return bad != 0;
}
void Engine::check_status() {
  if (poll_status())
    throw RangeError("non-finite value (inf / NaN) in the network output: an activation left the fp16 range of the matrix pipe (|x| > 65504) "
                     "or the input / weights were not finite; outputs of this frame are invalid");
}

void Engine::fetch_outputs() {
  if (!d_logits_) throw std::runtime_error("this engine has no outputs (batched encoder: fetch from its shared-prefix engines)");
  enqueue_fetch();
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
  check_status();
}

// D2H of the outputs the caller selected (vp_set_outputs), asynchronous on the engine stream, into pinned host memory.
void Engine::enqueue_fetch() {
  if (!d_logits_) throw std::runtime_error("this engine has no outputs (batched encoder: fetch from its shared-prefix engines)");
  if (outputs_ & 1)
    VP_HIP_CHECK(hipMemcpyAsync(h_logits_, d_logits_, (size_t)out_c_ * out_h_ * out_w_ * sizeof(float), hipMemcpyDeviceToHost, stream_));
  if ((outputs_ & 2) && d_mask_) VP_HIP_CHECK(hipMemcpyAsync(h_mask_, d_mask_, (size_t)out_h_ * out_w_, hipMemcpyDeviceToHost, stream_));
  host_logits_valid_ = (outputs_ & 1) != 0;
  host_mask_valid_ = (outputs_ & 2) != 0;
  if (finite_check_ && d_status_) {
    VP_HIP_CHECK(hipMemcpyAsync(h_status_, d_status_, VP_PROBE_BLOCKS * sizeof(unsigned), hipMemcpyDeviceToHost, stream_));
    status_pending_ = true;
  }
}

// The probe's verdict alone (vp_detect_infer: the network's output stays on the device; vp_logits fetches it lazily if asked)
void Engine::enqueue_status_fetch() {
  if (finite_check_ && d_status_) {
    VP_HIP_CHECK(hipMemcpyAsync(h_status_, d_status_, VP_PROBE_BLOCKS * sizeof(unsigned), hipMemcpyDeviceToHost, stream_));
    status_pending_ = true;
  }
}

// Lazy variants behind vp_logits / vp_mask_u8: an output de-selected with vp_set_outputs is fetched on first use.
const float* Engine::host_logits() {
  if (!host_logits_valid_ && d_logits_ && have_outputs_) {
    VP_HIP_CHECK(hipSetDevice(gpu_));
    VP_HIP_CHECK(hipMemcpyAsync(h_logits_, d_logits_, (size_t)out_c_ * out_h_ * out_w_ * sizeof(float), hipMemcpyDeviceToHost, stream_));
    VP_HIP_CHECK(hipStreamSynchronize(stream_));
    host_logits_valid_ = true;
  }
  return h_logits_;
}
const uint8_t* Engine::host_mask() {
  if (!host_mask_valid_ && d_mask_ && have_outputs_) {
    VP_HIP_CHECK(hipSetDevice(gpu_));
    VP_HIP_CHECK(hipMemcpyAsync(h_mask_, d_mask_, (size_t)out_h_ * out_w_, hipMemcpyDeviceToHost, stream_));
    VP_HIP_CHECK(hipStreamSynchronize(stream_));
    host_mask_valid_ = true;
  }
  return h_mask_;
}

void Engine::copy_outputs_device(void* logits_dst, void* mask_dst) {
  if (logits_dst)
    VP_HIP_CHECK(hipMemcpyAsync(logits_dst, d_logits_, (size_t)out_c_ * out_h_ * out_w_ * sizeof(float), hipMemcpyDeviceToDevice, stream_));
  if (mask_dst) VP_HIP_CHECK(hipMemcpyAsync(mask_dst, d_mask_, (size_t)out_h_ * out_w_, hipMemcpyDeviceToDevice, stream_));
}

void Engine::read_input_tensor(float* dst) {
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
  copy_d2h(dst, d_input_, (size_t)3 * net_h() * net_w() * sizeof(float));
}

// OpenCV resizeNN index table (oracle/pre_post.py nearest_index)
static void nearest_tab(int src, int dst, int* tab) {
  const double inv = (double)dst / (double)src;
  const double ifx = 1.0 / inv;
  for (int d = 0; d < dst; ++d) tab[d] = std::min((int)std::floor(d * ifx), src - 1);
}
static void linear_taps_f32(int src, int dst, int* idx, float* wgt) {
  const double scale = (double)src / (double)dst;
  for (int d = 0; d < dst; ++d) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)std::floor(f);
    f -= (float)s;
    if (s < 0) {
      f = 0.0f;
      s = 0;
    }
    if (s >= src - 1) {
      f = 0.0f;
      s = src - 1;
    }
    idx[2 * d] = s;
    idx[2 * d + 1] = std::min(s + 1, src - 1);
    wgt[2 * d] = 1.0f - f;
    wgt[2 * d + 1] = f;
  }
}

void Engine::mask_resized(uint8_t* dst, int h, int w) {
  if (!have_outputs_) throw std::runtime_error("Inference has not been run yet");
  if (!dst || h < 1 || w < 1) throw std::invalid_argument("bad resize target");
  const size_t need = (size_t)h * w, tabn = (size_t)(h + w);
  if (need > resize_cap_) {
    dfree(d_resize_out_);   // only this family of calls uses it, and each returns synchronised
    d_resize_out_ = dalloc(std::max(need, (size_t)4 * h * w), false);
    resize_cap_ = std::max(need, (size_t)4 * h * w);
  }
  if (tabn * 4 > rs_tab_cap_) {
    dfree(d_rs_tab_);
    d_rs_tab_ = static_cast<int*>(dalloc(tabn * 4 * sizeof(int), false));
    rs_tab_cap_ = tabn * 4;
  }
  std::vector<int> tab(h + w);
  nearest_tab(out_h_, h, tab.data());
  nearest_tab(out_w_, w, tab.data() + h);
  VP_HIP_CHECK(hipMemcpyAsync(d_rs_tab_, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
  VP_HIP_CHECK(launch_resize_nearest(d_mask_, out_w_, d_rs_tab_, d_rs_tab_ + h, h, w, static_cast<uint8_t*>(d_resize_out_), stream_));
  VP_HIP_CHECK(hipMemcpyAsync(dst, d_resize_out_, need, hipMemcpyDeviceToHost, stream_));
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
}

// createColorMask (masks_visualization_engine.cpp:41-58), BGR: [3 viz types][256][3]; label values not listed stay black
static std::vector<uint8_t> viz_color_lut() {
  std::vector<uint8_t> lut(3 * 256 * 3, 0);
  for (int v = 1; v < 256; ++v) { lut[(0 * 256 + v) * 3 + 2] = 255; }                          // "scene": 1..255 -> (0,0,255)
  const uint8_t dom0[3] = {255, 93, 61}, dom255[3] = {145, 28, 255};                            // "domain"
  for (int c = 0; c < 3; ++c) { lut[(1 * 256 + 0) * 3 + c] = dom0[c]; lut[(1 * 256 + 255) * 3 + c] = dom255[c]; }
  const uint8_t ego[3][3] = {{255, 0, 0}, {255, 0, 200}, {0, 153, 0}};                          // "egolanes": labels 0,1,2
  for (int v = 0; v < 3; ++v)
    for (int c = 0; c < 3; ++c) lut[(2 * 256 + v) * 3 + c] = ego[v][c];
  return lut;
}
static const uint8_t kViridisBgr[256 * 3] = {
#include "viridis_lut.inc"
};

// MasksVisualizationEngine::visualize on the device: the mask of the LAST inference, coloured, nearest-resized to the frame
// that produced it and blended 50/50 with that (still resident) frame; BGR8 out, frame size.
void Engine::visualize_mask(int viz_type, uint8_t* dst, int dst_h, int dst_w) {
  if (!have_outputs_) throw std::runtime_error("Inference has not been run yet");
  if (!dst || viz_type < 0 || viz_type > 2) throw std::invalid_argument("bad visualisation request");
  if (!d_frame_ || input_is_tensor_ || base_) throw std::runtime_error("visualize_mask needs the frame path (vp_infer) on a base engine");
  const int h = frame_h_, w = frame_w_;
  // The blend writes h*w*3 bytes: the caller's buffer must have the geometry of the frame that was inferred last (the
  // reference takes the size from original_image itself, masks_visualization_engine.cpp:19-27, so it cannot mismatch).
  if (dst_h != h || dst_w != w)
    throw std::invalid_argument("visualize_mask: destination is " + std::to_string(dst_w) + "x" + std::to_string(dst_h) +
                                " but the last inferred frame was " + std::to_string(w) + "x" + std::to_string(h));
  if (!d_viz_lut_) d_viz_lut_ = dupload(viz_color_lut());
  const size_t need = (size_t)3 * h * w, tabn = (size_t)(h + w);
  if (need > resize_cap_) {
    dfree(d_resize_out_);   // only this family of calls uses it, and each returns synchronised
    d_resize_out_ = dalloc(std::max(need, (size_t)4 * h * w), false);
    resize_cap_ = std::max(need, (size_t)4 * h * w);
  }
  if (tabn * 4 > rs_tab_cap_) {
    dfree(d_rs_tab_);
    d_rs_tab_ = static_cast<int*>(dalloc(tabn * 4 * sizeof(int), false));
    rs_tab_cap_ = tabn * 4;
  }
  std::vector<int> tab(h + w);
  nearest_tab(out_h_, h, tab.data());
  nearest_tab(out_w_, w, tab.data() + h);
  VP_HIP_CHECK(hipMemcpyAsync(d_rs_tab_, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
  VP_HIP_CHECK(launch_viz_blend(d_mask_, out_w_, d_rs_tab_, d_rs_tab_ + h, d_frame_, frame_stride_, h, w, d_viz_lut_ + (size_t)viz_type * 768,
                                pixel_format_ == 1, static_cast<uint8_t*>(d_resize_out_), stream_));
  VP_HIP_CHECK(hipMemcpyAsync(dst, d_resize_out_, need, hipMemcpyDeviceToHost, stream_));
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
}

void Engine::resize_depth_on_device(int h, int w) {
  const size_t need = (size_t)4 * h * w, tabn = (size_t)4 * (h + w);
  if (need > resize_cap_) {
    dfree(d_resize_out_);   // only this family of calls uses it, and each returns synchronised
    d_resize_out_ = dalloc(need, false);
    resize_cap_ = need;
  }
  if (tabn > rs_tab_cap_) {
    dfree(d_rs_tab_);
    d_rs_tab_ = static_cast<int*>(dalloc(tabn * sizeof(int), false));
    rs_tab_cap_ = tabn;
  }
  // host tap tables are members: they must outlive the asynchronous copies (every caller syncs the stream before returning)
  std::vector<int>& idx = rs_idx_host_;
  std::vector<float>& wgt = rs_wgt_host_;
  idx.assign(2 * (h + w), 0);
  wgt.assign(2 * (h + w), 0.f);
  linear_taps_f32(out_h_, h, idx.data(), wgt.data());
  linear_taps_f32(out_w_, w, idx.data() + 2 * h, wgt.data() + 2 * h);
  int* d_idx = d_rs_tab_;
  float* d_wgt = reinterpret_cast<float*>(d_rs_tab_ + 2 * (h + w));
  VP_HIP_CHECK(hipMemcpyAsync(d_idx, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
  VP_HIP_CHECK(hipMemcpyAsync(d_wgt, wgt.data(), wgt.size() * sizeof(float), hipMemcpyHostToDevice, stream_));
  VP_HIP_CHECK(launch_resize_bilinear_f32(d_logits_, out_w_, d_idx, d_wgt, d_idx + 2 * h, d_wgt + 2 * h, h, w,
                                          static_cast<float*>(d_resize_out_), stream_));
}

void Engine::depth_resized(float* dst, int h, int w) {
  if (!have_outputs_) throw std::runtime_error("Inference has not been run yet");
  if (!dst || h < 1 || w < 1) throw std::invalid_argument("bad resize target");
  resize_depth_on_device(h, w);
  VP_HIP_CHECK(hipMemcpyAsync(dst, d_resize_out_, (size_t)4 * h * w, hipMemcpyDeviceToHost, stream_));
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
}

// DepthVisualizationEngine::visualize (depth_visualization_engine.cpp:9-26) on the device: plane 0 of the logits,
// bilinear-resized to h x w (what the depth topic carries, run_model_node.cpp:100-104), min-max normalised to u8 and
// mapped through COLORMAP_VIRIDIS; BGR8 out.
void Engine::visualize_depth(uint8_t* dst, int h, int w) {
  if (!have_outputs_) throw std::runtime_error("Inference has not been run yet");
  if (!dst || h < 1 || w < 1) throw std::invalid_argument("bad visualisation target");
  if (!d_viridis_) {
    d_viridis_ = dupload(std::vector<uint8_t>(kViridisBgr, kViridisBgr + sizeof(kViridisBgr)));
    d_minmax_ = static_cast<unsigned*>(dalloc(2 * sizeof(unsigned), false));
  }
  const size_t n = (size_t)h * w;
  if (3 * n > depth_viz_cap_) {
    dfree(d_depth_viz_);
    d_depth_viz_ = dalloc(3 * n, false);
    depth_viz_cap_ = 3 * n;
  }
  resize_depth_on_device(h, w);
  static const unsigned kInit[2] = {0xFFFFFFFFu, 0u};
  VP_HIP_CHECK(hipMemcpyAsync(d_minmax_, kInit, sizeof(kInit), hipMemcpyHostToDevice, stream_));
  VP_HIP_CHECK(launch_minmax_f32(static_cast<const float*>(d_resize_out_), n, d_minmax_, stream_));
  VP_HIP_CHECK(launch_depth_colorize(static_cast<const float*>(d_resize_out_), n, d_minmax_, d_viridis_, static_cast<uint8_t*>(d_depth_viz_), stream_));
  VP_HIP_CHECK(hipMemcpyAsync(dst, d_depth_viz_, 3 * n, hipMemcpyDeviceToHost, stream_));
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
}

// -------------------------------------------------------------------------------------------------- vp_canvas
Canvas::Canvas(int gpu) : gpu_(gpu) {
  VP_HIP_CHECK(hipSetDevice(gpu_));
  try {
    VP_HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    for (hipEvent_t* ev : {&ev_src_, &ev_read_, &umask_ev_[0], &umask_ev_[1]}) VP_HIP_CHECK(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    std::vector<uint8_t> lut = viz_color_lut();
    lut.insert(lut.end(), kViridisBgr, kViridisBgr + sizeof(kViridisBgr));
    static const unsigned kKeys[4] = {0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u};
    VP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_lut_), lut.size()));
    VP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_minmax_), sizeof(kKeys)));
    VP_HIP_CHECK(hipMemcpyAsync(d_lut_, lut.data(), lut.size(), hipMemcpyHostToDevice, stream_));
    VP_HIP_CHECK(hipMemcpyAsync(d_minmax_, kKeys, sizeof(kKeys), hipMemcpyHostToDevice, stream_));
    VP_HIP_CHECK(hipStreamSynchronize(stream_));   // `lut` is a local
  } catch (...) {
    release();
    throw;
  }
}

Canvas::~Canvas() { release(); }

void Canvas::release() {
  (void)hipSetDevice(gpu_);
  if (stream_) (void)hipStreamSynchronize(stream_);
  for (hipEvent_t ev : {ev_src_, ev_read_, umask_ev_[0], umask_ev_[1]})
    if (ev) (void)hipEventDestroy(ev);
  for (const Table& t : tables_) {
    (void)hipFree(t.idx);
    if (t.wgt) (void)hipFree(t.wgt);
  }
  tables_.clear();
  for (void* p : {(void*)d_bgr_, (void*)d_lut_, (void*)d_minmax_, (void*)d_depth_, (void*)d_out_, (void*)d_small_, (void*)d_umask_})
    if (p) (void)hipFree(p);
  if (h_umask_) (void)hipHostFree(h_umask_);
  jpeg_.release();
  if (stream_) (void)hipStreamDestroy(stream_);
  stream_ = nullptr;
  ev_src_ = ev_read_ = umask_ev_[0] = umask_ev_[1] = nullptr;
  d_bgr_ = d_lut_ = d_out_ = d_small_ = d_umask_ = h_umask_ = nullptr;
  d_minmax_ = nullptr;
  d_depth_ = nullptr;
}

// a device buffer that has to grow is freed only once the canvas's own work has run
template <class T>
void Canvas::grow(T*& p, size_t& cap, size_t bytes) {
  if (bytes <= cap) return;
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
  if (p) (void)hipFree(p);
  p = nullptr;
  cap = 0;
  const size_t n = (bytes + 255) & ~(size_t)255;
  VP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&p), n));
  cap = n;
}

// The resize tables of visualize_mask / resize_depth_on_device (nearest_tab, linear_taps_f32) and of the preprocess path (linear_taps_u8), kept on the
// device per (kind, source, destination) size: the first use of a size uploads it and waits (the host vector is a local); every later draw finds it.  A
// handful of sizes per camera; the one unused longest goes when there are 16, so the two tables of one draw never push each other out.
Canvas::Table Canvas::table(TableKind kind, int src, int dst) {
  const bool linear = kind == kLinearF32;
  for (size_t i = 0; i < tables_.size(); ++i)
    if (tables_[i].kind == kind && tables_[i].src == src && tables_[i].dst == dst) {
      std::rotate(tables_.begin() + i, tables_.begin() + i + 1, tables_.end());
      return tables_.back();
    }
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
  if (tables_.size() >= 16) {
    (void)hipFree(tables_.front().idx);
    if (tables_.front().wgt) (void)hipFree(tables_.front().wgt);
    tables_.erase(tables_.begin());
  }
  Table t{kind, src, dst, nullptr, nullptr};
  std::vector<int> idx((linear ? 2 : 1) * (size_t)dst);
  std::vector<float> wgt;
  if (linear) {
    wgt.resize(2 * (size_t)dst);
    linear_taps_f32(src, dst, idx.data(), wgt.data());
  } else if (kind == kLinearU8) {
    linear_taps_u8(src, dst, &idx);
  } else {
    nearest_tab(src, dst, idx.data());
  }
  VP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&t.idx), idx.size() * sizeof(int)));
  tables_.push_back(t);   // owned from here on
  VP_HIP_CHECK(hipMemcpyAsync(t.idx, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
  if (linear) {
    VP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&tables_.back().wgt), wgt.size() * sizeof(float)));
    VP_HIP_CHECK(hipMemcpyAsync(tables_.back().wgt, wgt.data(), wgt.size() * sizeof(float), hipMemcpyHostToDevice, stream_));
  }
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
  return tables_.back();
}

void Canvas::need_begun(const char* who) const {
  if (!begun_) throw std::runtime_error(std::string(who) + ": the canvas holds no picture (vp_canvas_begin first)");
}

void Canvas::begin(const FrameView& f) {
  if (f.gpu != gpu_) throw std::invalid_argument("vp_canvas_begin: the frame lives on GPU " + std::to_string(f.gpu) + ", the canvas on GPU " + std::to_string(gpu_));
  if (!f.bgr) throw std::runtime_error("vp_canvas_begin: the frame was never uploaded (vp_frame_upload / vp_frame_upload_device first)");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  begun_ = false;
  grow(d_bgr_, bgr_cap_, (size_t)f.h * f.pitch);
  VP_HIP_CHECK(hipStreamWaitEvent(stream_, f.ready, 0));   // never a host wait: the copy runs once the frame's content is complete
  VP_HIP_CHECK(hipMemcpyAsync(d_bgr_, f.bgr, (size_t)f.h * f.pitch, hipMemcpyDeviceToDevice, stream_));   // same pitch on both sides: one copy
  h_ = f.h;
  w_ = f.w;
  pitch_ = f.pitch;
  begun_ = true;
}

// the refusals of blend_mask / paste_depth, the engine whose record counts (a head: its base) and the region the draw goes to
const Engine& Canvas::source_of(Engine& e, const char* who, SourceRegion* r, Draws draws) const {
  const std::string me(who);
  need_begun(who);
  if (e.gpu_ != gpu_) throw std::invalid_argument(me + ": the engine lives on GPU " + std::to_string(e.gpu_) + ", the canvas on GPU " + std::to_string(gpu_));
  if (draws == kLanePlanes && e.kind_ != 3) throw std::invalid_argument(me + ": VP_EGOLANES engines only (the three lane planes of its logits)");
  if (draws == kLaneRows && e.kind_ != 6) throw std::invalid_argument(me + ": VP_AUTOSTEER engines only (the lane rows xp / h_vector of its logits)");
  if (draws == kMaskOrDepth && (e.kind_ < 0 || e.kind_ > 3))
    throw std::invalid_argument(me + ": VP_AUTODRIVE / VP_AUTOSPEED / VP_AUTOSTEER engines have no mask or depth plane to draw");
  if (e.frames_ > 1) throw std::invalid_argument(me + ": a batched encoder has no outputs of its own (draw its per-camera heads)");
  if (!e.have_outputs_) throw std::runtime_error("Inference has not been run yet");
  const Engine& src = e.base_ ? *e.base_ : e;
  if (src.input_is_tensor_) throw std::invalid_argument(me + ": the engine's input was a tensor (vp_infer_tensor): there is no frame region to draw into");
  *r = src.src_region_;
  if (r->H != h_ || r->W != w_)
    throw std::invalid_argument(me + ": the engine's input came from a " + std::to_string(r->W) + " x " + std::to_string(r->H) + " frame, the canvas holds a " +
                                std::to_string(w_) + " x " + std::to_string(h_) + " picture");
  return src;
}

void Canvas::wait_for(Engine& e) {
  VP_HIP_CHECK(hipEventRecord(ev_src_, e.stream_));
  VP_HIP_CHECK(hipStreamWaitEvent(stream_, ev_src_, 0));
}
void Canvas::release_to(Engine& e) {
  VP_HIP_CHECK(hipEventRecord(ev_read_, stream_));
  VP_HIP_CHECK(hipStreamWaitEvent(e.stream_, ev_read_, 0));
}

void Canvas::blend(const uint8_t* d_mask, int mh, int mw, int viz_type, const SourceRegion& r) {
  const int* ytab = table(kNearest, mh, r.h).idx;
  const int* xtab = table(kNearest, mw, r.w).idx;
  CanvasBlendParams q{};
  q.mask = d_mask;
  q.mw = mw;
  q.ytab = ytab;
  q.xtab = xtab;
  q.lut = d_lut_ + (size_t)viz_type * 768;
  q.canvas = d_bgr_;
  q.pitch = pitch_;
  q.x0 = r.x0;
  q.y0 = r.y0;
  q.w = r.w;
  q.h = r.h;
  VP_HIP_CHECK(launch_canvas_blend(q, h_, w_, stream_));
}

void Canvas::blend_mask(Engine& e, int viz_type) {
  SourceRegion r;
  source_of(e, "vp_canvas_blend_mask", &r);
  if (viz_type < 0 || viz_type > 2) throw std::invalid_argument("vp_canvas_blend_mask: viz_type 0 (scene), 1 (domain) or 2 (egolanes)");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  wait_for(e);
  blend(e.d_mask_, e.out_h_, e.out_w_, viz_type, r);
  release_to(e);
}

void Canvas::blend_mask_u8(const uint8_t* mask, bool on_device, int mh, int mw, int viz_type, int x0, int y0, int w, int h) {
  need_begun("vp_canvas_blend_mask_u8");
  if (!mask || mh < 1 || mw < 1 || mh > 16384 || mw > 16384) throw std::invalid_argument("vp_canvas_blend_mask_u8: null mask or a mask size outside 1 .. 16384");
  if (viz_type < 0 || viz_type > 2) throw std::invalid_argument("vp_canvas_blend_mask_u8: viz_type 0 (scene), 1 (domain) or 2 (egolanes)");
  check_region("vp_canvas_blend_mask_u8", x0, y0, w, h);
  VP_HIP_CHECK(hipSetDevice(gpu_));
  const uint8_t* d_mask = on_device ? mask : stage_host(mask, (size_t)mh * mw);
  blend(d_mask, mh, mw, viz_type, SourceRegion{x0, y0, w, h, h_, w_});
}

void Canvas::check_region(const char* who, int x0, int y0, int w, int h) const {
  if (x0 < 0 || y0 < 0 || w < 2 || h < 2 || (long long)x0 + w > w_ || (long long)y0 + h > h_)
    throw std::invalid_argument(std::string(who) + ": region (x0 " + std::to_string(x0) + ", y0 " + std::to_string(y0) + ", " + std::to_string(w) + " x " + std::to_string(h) +
                                ") must be at least 2 x 2 and lie inside the " + std::to_string(w_) + " x " + std::to_string(h_) + " canvas");
}

// the caller's pageable array: copied into a pinned slot before the call returns, then one H2D
const uint8_t* Canvas::stage_host(const void* src, size_t n) {
  grow(d_umask_, umask_cap_, n);
  if (n > h_umask_cap_) {
    VP_HIP_CHECK(hipStreamSynchronize(stream_));
    if (h_umask_) (void)hipHostFree(h_umask_);
    h_umask_ = nullptr;
    h_umask_cap_ = 0;
    const size_t cap = (n + 255) & ~(size_t)255;
    VP_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&h_umask_), 2 * cap, hipHostMallocDefault));
    h_umask_cap_ = cap;
  }
  umask_slot_ ^= 1;
  uint8_t* slot = h_umask_ + (size_t)umask_slot_ * h_umask_cap_;
  VP_HIP_CHECK(hipEventSynchronize(umask_ev_[umask_slot_]));   // the H2D that last read this slot, two calls ago
  std::memcpy(slot, src, n);
  VP_HIP_CHECK(hipMemcpyAsync(d_umask_, slot, n, hipMemcpyHostToDevice, stream_));
  VP_HIP_CHECK(hipEventRecord(umask_ev_[umask_slot_], stream_));
  return d_umask_;
}

// ---- the production display's lanes: drawRawMasksInPlace's three additive overlays as one clamped sum per pixel
void Canvas::add(const float* d_planes, int n_planes, int mh, int mw, float threshold, const unsigned* add, const SourceRegion& r) {
  CanvasAddPlanesParams q{};
  q.planes = d_planes;
  q.n_planes = n_planes;
  q.plane_stride = mh * mw;
  q.mw = mw;
  q.ytab = table(kNearest, mh, r.h).idx;
  q.xtab = table(kNearest, mw, r.w).idx;
  q.threshold = threshold;
  for (int k = 0; k < n_planes; ++k) q.add[k] = add[k];
  q.canvas = d_bgr_;
  q.pitch = pitch_;
  q.x0 = r.x0;
  q.y0 = r.y0;
  q.w = r.w;
  q.h = r.h;
  VP_HIP_CHECK(launch_canvas_add_planes(q, h_, w_, stream_));
}

void Canvas::add_planes(const float* planes, bool on_device, int n_planes, int mh, int mw, float threshold, const uint8_t* add_bgr, int x0, int y0, int w, int h) {
  need_begun("vp_canvas_add_planes_f32");
  if (n_planes < 1 || n_planes > kCanvasMaxPlanes) throw std::invalid_argument("vp_canvas_add_planes_f32: n_planes " + std::to_string(n_planes) + " (1 .. 4)");
  if (!planes || !add_bgr) throw std::invalid_argument("vp_canvas_add_planes_f32: null planes or null add_bgr");
  if (mh < 1 || mw < 1 || mh > 16384 || mw > 16384) throw std::invalid_argument("vp_canvas_add_planes_f32: a plane size outside 1 .. 16384");
  if (!std::isfinite(threshold)) throw std::invalid_argument("vp_canvas_add_planes_f32: the threshold is not finite");
  check_region("vp_canvas_add_planes_f32", x0, y0, w, h);
  VP_HIP_CHECK(hipSetDevice(gpu_));
  unsigned add_px[kCanvasMaxPlanes];
  for (int k = 0; k < n_planes; ++k) add_px[k] = (unsigned)add_bgr[3 * k] | ((unsigned)add_bgr[3 * k + 1] << 8) | ((unsigned)add_bgr[3 * k + 2] << 16);
  const float* d_planes = on_device ? planes : reinterpret_cast<const float*>(stage_host(planes, (size_t)n_planes * mh * mw * sizeof(float)));
  add(d_planes, n_planes, mh, mw, threshold, add_px, SourceRegion{x0, y0, w, h, h_, w_});
}

void Canvas::overlay_lanes(Engine& e, float threshold) {
  SourceRegion r;
  source_of(e, "vp_canvas_overlay_lanes", &r, kLanePlanes);
  if (!std::isfinite(threshold)) throw std::invalid_argument("vp_canvas_overlay_lanes: the threshold is not finite");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  // rint(0.4 * colour) of drawRawMasksInPlace's colours, BGR, in plane order: ego left (255, 0, 0), ego right (255, 0, 200), other lanes (0, 153, 0)
  static const unsigned kAdd[3] = {102u, 102u | (80u << 16), 61u << 8};
  wait_for(e);
  add(e.d_logits_, 3, e.out_h_, e.out_w_, threshold, kAdd, r);
  release_to(e);
}

// ---- points
void Canvas::draw_points(const int* xy, int n, int radius, unsigned bgr) {
  need_begun("vp_canvas_draw_points");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  for (int first = 0; first < n; first += kCanvasPointChunk) {
    CanvasPointParams q{};
    q.canvas = d_bgr_;
    q.pitch = pitch_;
    q.radius = radius;
    q.bgr = bgr;
    q.ux0 = q.uy0 = INT_MAX;
    q.ux1 = q.uy1 = INT_MIN;
    for (int i = first; i < std::min(n, first + kCanvasPointChunk); ++i) {
      const long long x = xy[2 * i], y = xy[2 * i + 1];
      const long long cx0 = std::max(x - radius, 0ll), cy0 = std::max(y - radius, 0ll), cx1 = std::min(x + radius, (long long)w_ - 1), cy1 = std::min(y + radius, (long long)h_ - 1);
      if (cx1 < cx0 || cy1 < cy0) continue;   // wholly outside
      q.pt[q.n++] = CanvasPoint{(int)x, (int)y};
      q.ux0 = std::min(q.ux0, (int)cx0);
      q.uy0 = std::min(q.uy0, (int)cy0);
      q.ux1 = std::max(q.ux1, (int)cx1);
      q.uy1 = std::max(q.uy1, (int)cy1);
    }
    if (q.n) VP_HIP_CHECK(launch_canvas_points(q, h_, w_, stream_));
  }
}

// make_visualization (Models/visualizations/AutoSteer/video_visualization.py:19-44): which rows count is decided on the device, so the launch visits every
// pixel a valid row could reach: the rows oy - 3 .. oy + 511 + 3 of the canvas, all columns
void Canvas::draw_lane_rows(Engine& e) {
  SourceRegion r;
  source_of(e, "vp_canvas_draw_lane_rows", &r, kLaneRows);
  VP_HIP_CHECK(hipSetDevice(gpu_));
  CanvasPointParams q{};
  q.canvas = d_bgr_;
  q.pitch = pitch_;
  q.radius = 3;
  q.bgr = 0x00FF00u;
  q.n = e.out_h_;   // 64 rows
  q.rows = e.d_logits_;
  q.ox = r.x0;
  q.oy = r.y0;
  q.ux0 = 0;
  q.ux1 = w_ - 1;
  q.uy0 = std::max(r.y0 - q.radius, 0);
  q.uy1 = std::min(r.y0 + 511 + q.radius, h_ - 1);
  wait_for(e);
  VP_HIP_CHECK(launch_canvas_points(q, h_, w_, stream_));
  release_to(e);
}

// Engine::visualize_depth's pipeline at the region's size on the canvas's stream and buffers; only the last step differs: the colours go into the region
void Canvas::paste_depth(Engine& e) {
  SourceRegion r;
  source_of(e, "vp_canvas_paste_depth", &r);
  VP_HIP_CHECK(hipSetDevice(gpu_));
  const size_t n = (size_t)r.h * r.w;
  grow(d_depth_, depth_cap_, n * sizeof(float));
  const Table ty = table(kLinearF32, e.out_h_, r.h), tx = table(kLinearF32, e.out_w_, r.w);
  wait_for(e);
  VP_HIP_CHECK(launch_resize_bilinear_f32(e.d_logits_, e.out_w_, ty.idx, ty.wgt, tx.idx, tx.wgt, r.h, r.w, d_depth_, stream_));
  release_to(e);   // the logits are read: the engine's next pass may overwrite them
  VP_HIP_CHECK(hipMemcpyAsync(d_minmax_, d_minmax_ + 2, 2 * sizeof(unsigned), hipMemcpyDeviceToDevice, stream_));
  VP_HIP_CHECK(launch_minmax_f32(d_depth_, n, d_minmax_, stream_));
  VP_HIP_CHECK(launch_canvas_depth(d_depth_, d_minmax_, d_lut_ + 3 * 768, d_bgr_, pitch_, r.x0, r.y0, r.w, r.h, h_, w_, stream_));
}

void Canvas::draw_boxes(const CanvasBox* boxes, int n) {
  need_begun("vp_canvas_draw_detections");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  for (int first = 0; first < n; first += kCanvasBoxChunk) {
    CanvasBoxParams q{};
    q.canvas = d_bgr_;
    q.pitch = pitch_;
    q.ux0 = q.uy0 = INT_MAX;
    q.ux1 = q.uy1 = INT_MIN;
    for (int i = first; i < std::min(n, first + kCanvasBoxChunk); ++i) {
      const CanvasBox& b = boxes[i];
      const int cx0 = std::max(b.x0, 0), cy0 = std::max(b.y0, 0), cx1 = std::min(b.x1, w_ - 1), cy1 = std::min(b.y1, h_ - 1);
      if (cx1 < cx0 || cy1 < cy0) continue;   // empty, or wholly outside
      q.box[q.n++] = b;
      q.ux0 = std::min(q.ux0, cx0);
      q.uy0 = std::min(q.uy0, cy0);
      q.ux1 = std::max(q.ux1, cx1);
      q.uy1 = std::max(q.uy1, cy1);
    }
    if (q.n) VP_HIP_CHECK(launch_canvas_boxes(q, h_, w_, stream_));
  }
}

void Canvas::sync() {
  VP_HIP_CHECK(hipSetDevice(gpu_));
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
}

void Canvas::fetch(int format, uint8_t* const* planes, const int* strides, const size_t* row_bytes, const int* rows, int n_planes) {
  need_begun("vp_canvas_fetch");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  fetch_picture(d_bgr_, pitch_, h_, w_, format, planes, strides, row_bytes, rows, n_planes);
}

// cv::resize(unified_frame, display_frame, Size(1280, 720)) of the display thread (production_release/main.cpp:907), in the integer bilinear this library
// defines for the preprocess path; the result is a second picture, converted and copied by the path of fetch()
void Canvas::fetch_resized(int format, int out_h, int out_w, uint8_t* const* planes, const int* strides, const size_t* row_bytes, const int* rows, int n_planes) {
  need_begun("vp_canvas_fetch_resized");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  const int pitch = resize_to_small(out_h, out_w);
  fetch_picture(d_small_, pitch, out_h, out_w, format, planes, strides, row_bytes, rows, n_planes);
}

int Canvas::resize_to_small(int out_h, int out_w) {
  CanvasResizeParams q{};
  q.dst_pitch = frame_bgr_pitch(out_w);
  grow(d_small_, small_cap_, (size_t)out_h * q.dst_pitch);
  q.ytab = table(kLinearU8, h_, out_h).idx;
  q.xtab = table(kLinearU8, w_, out_w).idx;
  q.src = d_bgr_;
  q.src_pitch = pitch_;
  q.src_h = h_;
  q.src_w = w_;
  q.dst = d_small_;
  q.out_h = out_h;
  q.out_w = out_w;
  VP_HIP_CHECK(launch_canvas_resize(q, stream_));
  return q.dst_pitch;
}

void Canvas::fetch_picture(const uint8_t* d_bgr, int pitch, int h, int w, int format, uint8_t* const* planes, const int* strides, const size_t* row_bytes, const int* rows,
                           int n_planes) {
  if (format == VP_FRAME_BGR8) {
    VP_HIP_CHECK(hipMemcpy2DAsync(planes[0], strides[0], d_bgr, pitch, row_bytes[0], rows[0], hipMemcpyDeviceToHost, stream_));
  } else {
    const size_t pp = (size_t)canvas_plane_pitch(format, w), ppc = (size_t)canvas_plane_pitch(format, w, 1);   // both multiples of 4
    uint8_t* dev[3] = {nullptr, nullptr, nullptr};
    size_t off[4] = {0, 0, 0, 0};
    for (int i = 0; i < n_planes; ++i) off[i + 1] = off[i] + (i ? ppc : pp) * rows[i];
    grow(d_out_, out_cap_, off[n_planes]);
    for (int i = 0; i < n_planes; ++i) dev[i] = d_out_ + off[i];
    CanvasToFormatParams q{};
    q.src = d_bgr;
    q.src_pitch = pitch;
    q.h = h;
    q.w = w;
    q.format = format;
    q.p0 = dev[0];
    q.p1 = dev[1];
    q.p2 = dev[2];
    q.dst_pitch = (int)pp;
    q.dst_pitch_c = (int)ppc;
    q.chroma_mean = chroma_mode_;
    q.k = color_standard(matrix_, range_).fwd;
    VP_HIP_CHECK(launch_canvas_to_format(q, stream_));
    for (int i = 0; i < n_planes; ++i)
      VP_HIP_CHECK(hipMemcpy2DAsync(planes[i], strides[i], dev[i], i ? ppc : pp, row_bytes[i], rows[i], hipMemcpyDeviceToHost, stream_));
  }
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
}

void Canvas::fetch_jpeg(int out_h, int out_w, int quality, int restart_mcus, uint8_t* dst, size_t cap, size_t* n) {
  const char* who = out_h ? "vp_canvas_fetch_jpeg_resized" : "vp_canvas_fetch_jpeg";
  need_begun(who);
  VP_HIP_CHECK(hipSetDevice(gpu_));
  if (out_h) {
    const int pitch = resize_to_small(out_h, out_w);
    jpeg_.encode(d_small_, pitch, out_h, out_w, quality, restart_mcus, dst, cap, n, who, stream_);
  } else {
    jpeg_.encode(d_bgr_, pitch_, h_, w_, quality, restart_mcus, dst, cap, n, who, stream_);
  }
}

// -------------------------------------------------------------------------------------------------- baseline JPEG: the host half and the schedule
namespace {
// T.81 Annex K.1 / K.2, row-major
constexpr uint8_t kJpegBaseQ[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
constexpr uint8_t kJpegZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// T.81 Annex K.3.3: BITS[1 .. 16] and HUFFVAL of tables K.3 (DC luminance), K.5 (AC luminance), K.4 (DC chrominance), K.6 (AC chrominance) -- the DHT order
struct JpegHuffSpec {
  uint8_t bits[16];
  int n;
  uint8_t vals[162];
};
const JpegHuffSpec kJpegHuff[4] = {
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D},
     162,
     {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1,
      0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37,
      0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A,
      0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3,
      0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3,
      0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA}},
    {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
     162,
     {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1,
      0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36,
      0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
      0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A,
      0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA,
      0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA}}};

// the kernel's entries (code | length << 16, by symbol): [2][16] DC, then [2][256] AC; codes by T.81 Annex C
const uint32_t* jpeg_huff_words() {
  static const std::vector<uint32_t> words = [] {
    std::vector<uint32_t> w(kJpegHuffWords, 0u);
    for (int t = 0; t < 4; ++t) {
      uint32_t* dst = w.data() + ((t & 1) ? 32 + 256 * (t >> 1) : 16 * (t >> 1));
      unsigned code = 0;
      int k = 0;
      for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < kJpegHuff[t].bits[len - 1]; ++i) dst[kJpegHuff[t].vals[k++]] = code++ | ((unsigned)len << 16);
        code <<= 1;
      }
    }
    return w;
  }();
  return words.data();
}

uint8_t* jpeg_put_segment(uint8_t* p, int marker, int payload) {   // the marker and the length; the payload follows
  *p++ = 0xFF;
  *p++ = (uint8_t)marker;
  *p++ = (uint8_t)((payload + 2) >> 8);
  *p++ = (uint8_t)((payload + 2) & 255);
  return p;
}
}  // namespace

void jpeg_quant_tables(int quality, uint8_t q[2][64]) {
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i) q[t][i] = (uint8_t)std::min(std::max((kJpegBaseQ[t][i] * s + 50) / 100, 1), 255);
}

// Per MCU six blocks of at most 22 + 63 * 26 bits: the longest DC code (11 bits) + 11, and per AC position at most the longest code (16 bits) + 10 -- a ZRL
// or an EOB is shorter than the coefficients it stands for.  That is 1245 whole bytes, so an interval's padding stays inside them; every byte may be
// stuffed; + 2 per interval for its marker.
size_t jpeg_scan_bound(int h, int w, int restart_mcus) {
  const size_t n = (size_t)((h + 15) / 16) * ((w + 15) / 16), ri = (size_t)jpeg_restart(restart_mcus);
  return n * 2 * (6 * (22 + 63 * 26) / 8) + 2 * ((n + ri - 1) / ri);
}

void jpeg_write_header(int h, int w, int quality, int restart_mcus, uint8_t dst[kJpegHeaderBytes]) {
  uint8_t q[2][64];
  jpeg_quant_tables(quality, q);
  uint8_t* p = dst;
  *p++ = 0xFF;
  *p++ = 0xD8;
  p = jpeg_put_segment(p, 0xE0, 14);
  for (uint8_t b : {0x4A, 0x46, 0x49, 0x46, 0x00, 1, 1, 0, 0, 1, 0, 1, 0, 0}) *p++ = b;   // "JFIF\0", 1.01, no units, 1:1, no thumbnail
  for (int t = 0; t < 2; ++t) {
    p = jpeg_put_segment(p, 0xDB, 65);
    *p++ = (uint8_t)t;
    for (int i = 0; i < 64; ++i) *p++ = q[t][kJpegZigzag[i]];
  }
  p = jpeg_put_segment(p, 0xC0, 15);
  for (int b : {8, h >> 8, h & 255, w >> 8, w & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1}) *p++ = (uint8_t)b;
  for (int t = 0; t < 4; ++t) {
    p = jpeg_put_segment(p, 0xC4, 17 + kJpegHuff[t].n);
    *p++ = (uint8_t)(((t & 1) << 4) | (t >> 1));
    for (int i = 0; i < 16; ++i) *p++ = kJpegHuff[t].bits[i];
    for (int i = 0; i < kJpegHuff[t].n; ++i) *p++ = kJpegHuff[t].vals[i];
  }
  const int ri = jpeg_restart(restart_mcus);
  p = jpeg_put_segment(p, 0xDD, 2);
  *p++ = (uint8_t)(ri >> 8);
  *p++ = (uint8_t)(ri & 255);
  p = jpeg_put_segment(p, 0xDA, 10);
  for (uint8_t b : {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0}) *p++ = b;
  if ((size_t)(p - dst) != kJpegHeaderBytes) throw std::logic_error("jpeg_write_header: the header's length");
}

void JpegEncoder::release() {
  for (void* p : {(void*)d_coef_, (void*)d_len_, (void*)d_out_, (void*)d_huff_})
    if (p) (void)hipFree(p);
  if (h_total_) (void)hipHostFree(h_total_);
  d_coef_ = nullptr;
  d_len_ = nullptr;
  d_out_ = nullptr;
  d_huff_ = nullptr;
  h_total_ = nullptr;
  coef_cap_ = len_cap_ = out_cap_ = 0;
}

// as Canvas::grow: a buffer that has to grow is freed only once the stream's work has run
void JpegEncoder::grow(void** p, size_t* cap, size_t bytes, hipStream_t st) {
  if (bytes <= *cap) return;
  VP_HIP_CHECK(hipStreamSynchronize(st));
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  const size_t n = (bytes + 255) & ~(size_t)255;
  VP_HIP_CHECK(hipMalloc(p, n));
  *cap = n;
}

void JpegEncoder::encode(const uint8_t* d_bgr, int pitch, int h, int w, int quality, int restart_mcus, uint8_t* dst, size_t cap, size_t* n, const char* who,
                         hipStream_t st) {
  const int ri = jpeg_restart(restart_mcus), mcus_x = (w + 15) / 16, n_mcus = mcus_x * ((h + 15) / 16), n_int = (n_mcus + ri - 1) / ri;
  grow(reinterpret_cast<void**>(&d_coef_), &coef_cap_, (size_t)n_mcus * 6 * 64 * sizeof(int16_t), st);
  grow(reinterpret_cast<void**>(&d_len_), &len_cap_, (size_t)n_mcus * sizeof(uint32_t), st);
  grow(reinterpret_cast<void**>(&d_out_), &out_cap_, jpeg_scan_bound(h, w, 1), st);   // restart_mcus = 1 has the largest bound: one size per geometry
  if (!d_huff_) {
    VP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_huff_), kJpegHuffWords * sizeof(uint32_t)));
    VP_HIP_CHECK(hipMemcpyAsync(d_huff_, jpeg_huff_words(), kJpegHuffWords * sizeof(uint32_t), hipMemcpyHostToDevice, st));   // the source is static
  }
  if (!h_total_) VP_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&h_total_), 64, hipHostMallocDefault));
  if (cap >= kJpegHeaderBytes) jpeg_write_header(h, w, quality, restart_mcus, dst);
  JpegBlocksParams b{};
  b.src = d_bgr;
  b.src_pitch = pitch;
  b.h = h;
  b.w = w;
  b.mcus_x = mcus_x;
  b.n_mcus = n_mcus;
  b.k = color_standard(VP_COLOR_BT601, VP_COLOR_RANGE_FULL).fwd;   // JFIF's standard, whatever vp_canvas_set_color says
  jpeg_quant_tables(quality, b.q);
  b.coef = d_coef_;
  JpegEntropyParams e{};
  e.coef = d_coef_;
  e.huff = d_huff_;
  e.n_mcus = n_mcus;
  e.restart_mcus = ri;
  e.n_intervals = n_int;
  e.len = d_len_;
  e.out = d_out_;
  VP_HIP_CHECK(launch_jpeg_blocks(b, st));
  VP_HIP_CHECK(launch_jpeg_entropy(e, false, st));
  VP_HIP_CHECK(launch_jpeg_scan(d_len_, n_int, h_total_, st));
  VP_HIP_CHECK(launch_jpeg_entropy(e, true, st));
  VP_HIP_CHECK(hipStreamSynchronize(st));   // wait 1: the total
  const size_t total = *h_total_, need = kJpegHeaderBytes + total + 2;
  if (cap < need) {
    *n = need;
    throw std::invalid_argument(std::string(who) + ": the stream has " + std::to_string(need) + " bytes, cap is " + std::to_string(cap));
  }
  VP_HIP_CHECK(hipMemcpyAsync(dst + kJpegHeaderBytes, d_out_, total, hipMemcpyDeviceToHost, st));
  VP_HIP_CHECK(hipStreamSynchronize(st));   // wait 2: the stream
  dst[kJpegHeaderBytes + total] = 0xFF;
  dst[kJpegHeaderBytes + total + 1] = 0xD9;
  *n = need;
}

// -------------------------------------------------------------------------------------------------- vp_metric
Metric::Metric(int gpu, int max_frames) : gpu_(gpu), max_frames_(max_frames) {
  if (max_frames < 1 || max_frames > (1 << 20)) throw std::invalid_argument("vp_metric_create: max_frames " + std::to_string(max_frames) + " (1 .. 1048576)");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  try {
    VP_HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    for (hipEvent_t* ev : {&ev_src_[0], &ev_src_[1], &ev_read_[0], &ev_read_[1], &stage_[0].ev[0], &stage_[0].ev[1], &stage_[1].ev[0], &stage_[1].ev[1]})
      VP_HIP_CHECK(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    VP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_records_), (size_t)max_frames * sizeof(MetricRecord)));
    VP_HIP_CHECK(hipMemsetAsync(d_records_, 0, (size_t)max_frames * sizeof(MetricRecord), stream_));
  } catch (...) {
    release();
    throw;
  }
}

Metric::~Metric() { release(); }

void Metric::release() {
  (void)hipSetDevice(gpu_);
  if (stream_) (void)hipStreamSynchronize(stream_);
  for (hipEvent_t* ev : {&ev_src_[0], &ev_src_[1], &ev_read_[0], &ev_read_[1], &stage_[0].ev[0], &stage_[0].ev[1], &stage_[1].ev[0], &stage_[1].ev[1]}) {
    if (*ev) (void)hipEventDestroy(*ev);
    *ev = nullptr;
  }
  for (Stage& s : stage_) {
    if (s.d) (void)hipFree(s.d);
    if (s.h) (void)hipHostFree(s.h);
    s.d = s.h = nullptr;
    s.dcap = s.hcap = 0;
  }
  if (d_records_) (void)hipFree(d_records_);
  if (d_scratch_) (void)hipFree(d_scratch_);
  d_records_ = nullptr;
  d_scratch_ = nullptr;
  scratch_cap_ = 0;
  for (hipEvent_t& ev : det_stage_.ev) {
    if (ev) (void)hipEventDestroy(ev);
    ev = nullptr;
  }
  if (det_stage_.d) (void)hipFree(det_stage_.d);
  if (det_stage_.h) (void)hipHostFree(det_stage_.h);
  det_stage_.d = det_stage_.h = nullptr;
  det_stage_.dcap = det_stage_.hcap = 0;
  for (void** p : {reinterpret_cast<void**>(&d_det_frames_), reinterpret_cast<void**>(&d_det_rows_), reinterpret_cast<void**>(&d_det_label_cls_),
                   reinterpret_cast<void**>(&d_det_small_), reinterpret_cast<void**>(&d_det_scratch_)}) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
  det_scratch_cap_ = 0;
  for (void** p : {reinterpret_cast<void**>(&d_lanes_records_), reinterpret_cast<void**>(&d_rows_records_), reinterpret_cast<void**>(&d_lanes_scratch_)}) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
  lanes_scratch_cap_ = 0;
  for (void** p : {reinterpret_cast<void**>(&d_label_records_), reinterpret_cast<void**>(&d_label_scratch_)}) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
  label_scratch_cap_ = 0;
  for (LabelTab& t : label_tabs_) (void)hipFree(t.idx);
  label_tabs_.clear();
  if (stream_) (void)hipStreamDestroy(stream_);
  stream_ = nullptr;
}

// behind everything queued so far: the used records become zero again (the segmentation kernel adds into its record)
void Metric::reset() {
  VP_HIP_CHECK(hipSetDevice(gpu_));
  if (frames_) VP_HIP_CHECK(hipMemsetAsync(d_records_, 0, (size_t)frames_ * sizeof(MetricRecord), stream_));
  frames_ = 0;
  if (d_det_small_) VP_HIP_CHECK(hipMemsetAsync(d_det_small_, 0, 2 * sizeof(unsigned), stream_));   // the running totals
  det_frames_ = det_n_iou_ = 0;
  det_labels_bound_ = 0;
  lanes_frames_ = rows_lines_ = rows_n_thr_ = label_frames_ = 0;   // their kernels store whole records
}

// a device buffer that has to grow is freed only once the metric's own work has run
template <class T>
void Metric::grow(T*& p, size_t& cap, size_t bytes) {
  if (bytes <= cap) return;
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
  if (p) (void)hipFree(p);
  p = nullptr;
  cap = 0;
  const size_t n = (bytes + 255) & ~(size_t)255;
  VP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&p), n));
  cap = n;
}

// Canvas::stage_host's scheme, one Stage per argument
const void* Metric::stage_host(Stage& s, const void* src, size_t n) {
  grow(s.d, s.dcap, n);
  if (n > s.hcap) {
    VP_HIP_CHECK(hipStreamSynchronize(stream_));
    if (s.h) (void)hipHostFree(s.h);
    s.h = nullptr;
    s.hcap = 0;
    const size_t cap = (n + 255) & ~(size_t)255;
    VP_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&s.h), 2 * cap, hipHostMallocDefault));
    s.hcap = cap;
  }
  s.slot ^= 1;
  uint8_t* slot = s.h + (size_t)s.slot * s.hcap;
  VP_HIP_CHECK(hipEventSynchronize(s.ev[s.slot]));   // the H2D that last read this slot, two calls ago
  std::memcpy(slot, src, n);
  VP_HIP_CHECK(hipMemcpyAsync(s.d, slot, n, hipMemcpyHostToDevice, stream_));
  VP_HIP_CHECK(hipEventRecord(s.ev[s.slot], stream_));
  return s.d;
}

// the refusals of the engine entries; the engine itself is the source (a head has logits of its own)
const Engine& Metric::source_of(Engine& e, const char* who, bool depth) const {
  const std::string me(who);
  if (e.gpu_ != gpu_) throw std::invalid_argument(me + ": the engine lives on GPU " + std::to_string(e.gpu_) + ", the metric on GPU " + std::to_string(gpu_));
  if (depth ? e.kind_ != 1 : (e.kind_ != 0 && e.kind_ != 2))
    throw std::invalid_argument(me + (depth ? ": VP_SCENE3D engines only (plane 0 of its logits is the depth map)" : ": VP_SCENESEG and VP_DOMAINSEG engines only"));
  if (e.frames_ > 1) throw std::invalid_argument(me + ": a batched encoder has no outputs of its own (score its per-camera heads)");
  if (!e.have_outputs_) throw std::runtime_error("Inference has not been run yet");
  if (!e.d_logits_ || (e.out_c_ != 1 && e.out_c_ != 3) || e.out_h_ < 1 || e.out_w_ < 1) throw std::invalid_argument(me + ": the engine has no logits of one or three planes");
  return e;
}

void Metric::wait_for(Engine& e, hipEvent_t ev) {
  VP_HIP_CHECK(hipEventRecord(ev, e.stream_));
  VP_HIP_CHECK(hipStreamWaitEvent(stream_, ev, 0));
}
void Metric::release_to(Engine& e, hipEvent_t ev) {
  VP_HIP_CHECK(hipEventRecord(ev, stream_));
  VP_HIP_CHECK(hipStreamWaitEvent(e.stream_, ev, 0));
}

MetricRecord* Metric::next_record(const char* who) {
  if (frames_ >= max_frames_) throw std::runtime_error(std::string(who) + ": the accumulator is full (" + std::to_string(max_frames_) + " frames; vp_metric_fetch, then vp_metric_reset)");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  return d_records_ + frames_;
}

void Metric::seg(const float* d_logits, const float* d_ref, const uint8_t* d_gt, int c, int h, int w, int gt_form, MetricRecord* rec) {
  MetricSegParams q{};   // the record's counters are zero: the constructor and reset() leave every unused record so
  q.logits = d_logits;
  q.ref = d_ref;
  q.gt = d_gt;
  q.c = c;
  q.gt_form = gt_form;
  q.kind = c == 3 ? 0 : 2;   // VP_SCENESEG : VP_DOMAINSEG
  q.n = (unsigned)h * (unsigned)w;
  q.rec = rec;
  VP_HIP_CHECK(launch_metric_seg_count(q, stream_));
}

void Metric::depth(const float* d_pred, const float* d_gt, int h, int w, MetricRecord* rec) {
  const size_t n = (size_t)h * w, pe = metric_pooled_elems(h, w);
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t o_a = up(4 * n), o_pool = o_a + up(4 * n), o_stat = o_pool + up(4 * pe), o_kept = o_stat + up(kMetricBlocks * sizeof(MetricStatPartial)),
               o_edge = o_kept + up(kMetricBlocks * sizeof(MetricKeptPartial)), o_sel = o_edge + up(4 * kMetricBlocks * sizeof(double)), o_ssc = o_sel + 256, total = o_ssc + up(metric_select_scratch_bytes((unsigned)n));
  grow(d_scratch_, scratch_cap_, total);
  MetricDepthParams q{};
  q.pred = d_pred;
  q.gt = d_gt;
  q.h = h;
  q.w = w;
  q.kind = 1;   // VP_SCENE3D
  q.d = reinterpret_cast<float*>(d_scratch_);
  q.a_bits = reinterpret_cast<unsigned*>(d_scratch_ + o_a);
  q.pooled = reinterpret_cast<float*>(d_scratch_ + o_pool);
  q.stat = reinterpret_cast<MetricStatPartial*>(d_scratch_ + o_stat);
  q.kept = reinterpret_cast<MetricKeptPartial*>(d_scratch_ + o_kept);
  q.edge = reinterpret_cast<double*>(d_scratch_ + o_edge);
  q.sel = reinterpret_cast<unsigned*>(d_scratch_ + o_sel);
  q.sel_scratch = reinterpret_cast<unsigned*>(d_scratch_ + o_ssc);
  q.rec = rec;
  VP_HIP_CHECK(launch_metric_depth(q, stream_));
}

static void metric_check_seg_args(const char* who, const void* logits, int c, int h, int w, const void* gt, int gt_form) {
  const std::string me(who);
  if (!logits || !gt) throw std::invalid_argument(me + ": null logits or null ground truth");
  if (c != 1 && c != 3) throw std::invalid_argument(me + ": c " + std::to_string(c) + " (1: DomainSeg, 3: SceneSeg)");
  if (h < 1 || w < 1 || (long long)h * w > (long long)kMetricMaxN) throw std::invalid_argument(me + ": h * w outside 1 .. 2^24");
  if (gt_form != 0 && gt_form != 1) throw std::invalid_argument(me + ": gt_form " + std::to_string(gt_form) + " (VP_GT_LABEL, VP_GT_BITS)");
}
static void metric_check_depth_args(const char* who, const void* pred, const void* gt, int h, int w) {
  const std::string me(who);
  if (!pred || !gt) throw std::invalid_argument(me + ": null prediction or null ground truth");
  if (h < 8 || w < 8) throw std::invalid_argument(me + ": a plane of " + std::to_string(h) + " x " + std::to_string(w) + " (the three 2x2 pools need 8 x 8 at least)");
  if ((long long)h * w > (long long)kMetricMaxN) throw std::invalid_argument(me + ": h * w above 2^24");
}

void Metric::add_seg(Engine& e, const uint8_t* gt, bool gt_on_device, int gt_form) {
  source_of(e, "vp_metric_add_seg", false);
  metric_check_seg_args("vp_metric_add_seg", e.d_logits_, e.out_c_, e.out_h_, e.out_w_, gt, gt_form);
  MetricRecord* rec = next_record("vp_metric_add_seg");
  const uint8_t* d_gt = gt_on_device ? gt : static_cast<const uint8_t*>(stage_host(stage_[1], gt, (size_t)e.out_h_ * e.out_w_));
  wait_for(e, ev_src_[0]);
  seg(e.d_logits_, nullptr, d_gt, e.out_c_, e.out_h_, e.out_w_, gt_form, rec);
  release_to(e, ev_read_[0]);
  ++frames_;
}

void Metric::add_depth(Engine& e, const float* gt, bool gt_on_device) {
  source_of(e, "vp_metric_add_depth", true);
  metric_check_depth_args("vp_metric_add_depth", e.d_logits_, gt, e.out_h_, e.out_w_);
  MetricRecord* rec = next_record("vp_metric_add_depth");
  const float* d_gt = gt_on_device ? gt : static_cast<const float*>(stage_host(stage_[1], gt, sizeof(float) * (size_t)e.out_h_ * e.out_w_));
  wait_for(e, ev_src_[0]);
  depth(e.d_logits_, d_gt, e.out_h_, e.out_w_, rec);
  release_to(e, ev_read_[0]);
  ++frames_;
}

void Metric::add_seg_pair(Engine& e, Engine& ref) {
  source_of(e, "vp_metric_add_seg_pair", false);
  source_of(ref, "vp_metric_add_seg_pair", false);
  if (e.kind_ != ref.kind_ || e.out_c_ != ref.out_c_ || e.out_h_ != ref.out_h_ || e.out_w_ != ref.out_w_)
    throw std::invalid_argument("vp_metric_add_seg_pair: the two engines are of different kinds or output sizes");
  metric_check_seg_args("vp_metric_add_seg_pair", e.d_logits_, e.out_c_, e.out_h_, e.out_w_, ref.d_logits_, 0);
  MetricRecord* rec = next_record("vp_metric_add_seg_pair");
  wait_for(e, ev_src_[0]);
  if (&ref != &e) wait_for(ref, ev_src_[1]);
  seg(e.d_logits_, ref.d_logits_, nullptr, e.out_c_, e.out_h_, e.out_w_, 0, rec);
  release_to(e, ev_read_[0]);
  if (&ref != &e) release_to(ref, ev_read_[1]);
  ++frames_;
}

void Metric::add_depth_pair(Engine& e, Engine& ref) {
  source_of(e, "vp_metric_add_depth_pair", true);
  source_of(ref, "vp_metric_add_depth_pair", true);
  if (e.out_h_ != ref.out_h_ || e.out_w_ != ref.out_w_) throw std::invalid_argument("vp_metric_add_depth_pair: the two engines are of different output sizes");
  metric_check_depth_args("vp_metric_add_depth_pair", e.d_logits_, ref.d_logits_, e.out_h_, e.out_w_);
  MetricRecord* rec = next_record("vp_metric_add_depth_pair");
  wait_for(e, ev_src_[0]);
  if (&ref != &e) wait_for(ref, ev_src_[1]);
  depth(e.d_logits_, ref.d_logits_, e.out_h_, e.out_w_, rec);
  release_to(e, ev_read_[0]);
  if (&ref != &e) release_to(ref, ev_read_[1]);
  ++frames_;
}

void Metric::add_seg_logits(const float* logits, bool on_device, int c, int h, int w, const uint8_t* gt, bool gt_on_device, int gt_form) {
  metric_check_seg_args("vp_metric_add_seg_logits", logits, c, h, w, gt, gt_form);
  MetricRecord* rec = next_record("vp_metric_add_seg_logits");
  const size_t n = (size_t)h * w;
  const float* d_logits = on_device ? logits : static_cast<const float*>(stage_host(stage_[0], logits, sizeof(float) * n * c));
  const uint8_t* d_gt = gt_on_device ? gt : static_cast<const uint8_t*>(stage_host(stage_[1], gt, n));
  if (reinterpret_cast<uintptr_t>(d_logits) & 3) throw std::invalid_argument("vp_metric_add_seg_logits: device logits not aligned to 4 bytes");
  seg(d_logits, nullptr, d_gt, c, h, w, gt_form, rec);
  ++frames_;
}

void Metric::add_depth_plane(const float* pred, bool pred_on_device, const float* gt, bool gt_on_device, int h, int w) {
  metric_check_depth_args("vp_metric_add_depth_plane", pred, gt, h, w);
  MetricRecord* rec = next_record("vp_metric_add_depth_plane");
  const size_t bytes = sizeof(float) * (size_t)h * w;
  const float* d_pred = pred_on_device ? pred : static_cast<const float*>(stage_host(stage_[0], pred, bytes));
  const float* d_gt = gt_on_device ? gt : static_cast<const float*>(stage_host(stage_[1], gt, bytes));
  if ((reinterpret_cast<uintptr_t>(d_pred) | reinterpret_cast<uintptr_t>(d_gt)) & 3) throw std::invalid_argument("vp_metric_add_depth_plane: device planes not aligned to 4 bytes");
  depth(d_pred, d_gt, h, w, rec);
  ++frames_;
}

void Metric::fetch(MetricRecord* out, int count) {
  if (count < 0 || count > frames_ || (count > 0 && !out)) throw std::invalid_argument("vp_metric_fetch: more records than were added, or a null buffer");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  if (count) VP_HIP_CHECK(hipMemcpyAsync(out, d_records_, (size_t)count * sizeof(MetricRecord), hipMemcpyDeviceToHost, stream_));
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
}

// ---- the detector part: records, rows and label classes of their own, allocated by the first add_det*
namespace {
// d_det_small_: totals [2] | set 0 {rows [300][7], counts [3]} | set 1 (the pair form's reference chain) | pair labels [300][5] | their count
constexpr size_t kDetSmallRows = 8448, kDetSmallSet = kDetSmallRows + 256, kDetSmallLabels = 256 + 2 * kDetSmallSet, kDetSmallBytes = kDetSmallLabels + 6144 + 256;
static_assert(kDetSmallRows >= (size_t)kDetValMaxDet * kDetValRowWords * sizeof(float) && 6144 >= (size_t)kDetValMaxDet * 5 * sizeof(float), "d_det_small_ layout");
}  // namespace

const Engine& Metric::det_source_of(Engine& e, const char* who) const {
  const std::string me(who);
  if (e.gpu_ != gpu_) throw std::invalid_argument(me + ": the engine lives on GPU " + std::to_string(e.gpu_) + ", the metric on GPU " + std::to_string(gpu_));
  if (e.kind_ != 5) throw std::invalid_argument(me + ": VP_AUTOSPEED engines only");
  if (!e.have_outputs_) throw std::runtime_error("Inference has not been run yet");
  if (!e.d_logits_ || e.out_c_ < 5 || e.out_w_ < 1) throw std::invalid_argument(me + ": the engine has no raw detector tensor");
  return e;
}

void Metric::det_begin(const char* who, int nc, int nb, int n_labels_bound, const float* iou_v, int n_iou, float conf, float iou) {
  const std::string me(who);
  if (nc < 1 || nc > kDetValMaxClasses || nb < 1 || nb > kDetValMaxBoxes || (long long)nb * nc > (long long)kDetValMaxPairs)
    throw std::invalid_argument(me + ": nc " + std::to_string(nc) + ", nb " + std::to_string(nb) + " (nc 1 .. 80, nb 1 .. 16384, nb * nc <= 131072)");
  if (!iou_v || n_iou < 1 || n_iou > kDetValMaxIou) throw std::invalid_argument(me + ": a null threshold table, or n_iou outside 1 .. 16");
  if (n_labels_bound < 0 || n_labels_bound > kDetValMaxLabels) throw std::invalid_argument(me + ": n_labels outside 0 .. 4096");
  if (conf != conf || iou != iou) throw std::invalid_argument(me + ": a NaN threshold");
  if (det_frames_ && (n_iou != det_n_iou_ || std::memcmp(iou_v, det_iou_v_, sizeof(float) * (size_t)n_iou) != 0))
    throw std::invalid_argument(me + ": another threshold table than the records added so far were matched with (vp_metric_reset first)");
  const size_t label_cap = (size_t)det_capacity() * kDetLabelsPerFrame + kDetValMaxLabels;
  if (det_frames_ >= det_capacity() || det_labels_bound_ + (size_t)n_labels_bound > label_cap)
    throw std::runtime_error(me + ": the detector accumulator is full (" + std::to_string(det_capacity()) + " frames, " + std::to_string(label_cap) + " labels; vp_metric_fetch_det, then vp_metric_reset)");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  if (!d_det_small_) {   // allocated last: a failure half way is cleaned up by the next attempt or by release()
    for (void** p : {reinterpret_cast<void**>(&d_det_frames_), reinterpret_cast<void**>(&d_det_rows_), reinterpret_cast<void**>(&d_det_label_cls_)}) {
      if (*p) (void)hipFree(*p);
      *p = nullptr;
    }
    for (hipEvent_t& ev : det_stage_.ev)
      if (!ev) VP_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    const size_t cap = (size_t)det_capacity();
    VP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_det_frames_), cap * sizeof(DetFrameRecord)));
    VP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_det_rows_), cap * kDetValMaxDet * sizeof(DetRowRecord)));
    VP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_det_label_cls_), label_cap * sizeof(float)));
    uint8_t* small = nullptr;
    VP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&small), kDetSmallBytes));
    if (hipError_t err = hipMemsetAsync(small, 0, kDetSmallBytes, stream_); err != hipSuccess) {
      (void)hipFree(small);
      VP_HIP_CHECK(err);
    }
    d_det_small_ = small;
  }
  det_n_iou_ = n_iou;
  std::memcpy(det_iou_v_, iou_v, sizeof(float) * (size_t)n_iou);
}

DetValParams Metric::det_chain(const float* d_raw, int nc, int nb, float conf, float iou, int which) {
  grow(d_det_scratch_, det_scratch_cap_, det_val_scratch_bytes((unsigned)nb, (unsigned)nc));
  DetValParams q{};
  q.raw = d_raw;
  q.nb = (unsigned)nb;
  q.nc = (unsigned)nc;
  q.conf = conf;
  q.iou = iou;
  q.max_nms = kDetValMaxNms;
  q.max_det = kDetValMaxDet;
  det_val_carve(d_det_scratch_, &q);
  uint8_t* set = d_det_small_ + 256 + (size_t)which * kDetSmallSet;
  q.rows = reinterpret_cast<float*>(set);
  q.counts = reinterpret_cast<unsigned*>(set + kDetSmallRows);
  VP_HIP_CHECK(launch_det_validate(q, stream_));
  return q;
}

void Metric::det_match(const float* d_labels, const unsigned* d_n_labels, int n_labels, int label_form, int net_h, int net_w) {
  DetMatchParams q{};
  q.rows = reinterpret_cast<const float*>(d_det_small_ + 256);
  q.counts = reinterpret_cast<const unsigned*>(d_det_small_ + 256 + kDetSmallRows);
  q.labels = d_labels;
  q.n_labels_dev = d_n_labels;
  q.n_labels = n_labels;
  q.label_form = label_form;
  q.W = (float)net_w;
  q.H = (float)net_h;
  std::memcpy(q.iou_v, det_iou_v_, sizeof(q.iou_v));
  q.n_iou = det_n_iou_;
  q.totals = reinterpret_cast<unsigned*>(d_det_small_);
  q.frame = d_det_frames_ + det_frames_;
  q.rows_out = d_det_rows_;
  q.label_cls_out = d_det_label_cls_;
  VP_HIP_CHECK(launch_det_val_match(q, stream_));
  ++det_frames_;
  det_labels_bound_ += (size_t)n_labels;
}

void Metric::add_det(Engine& e, const float* labels, int n_labels, float conf, float iou, const float* iou_v, int n_iou) {
  det_source_of(e, "vp_metric_add_det");
  if (n_labels > 0 && !labels) throw std::invalid_argument("vp_metric_add_det: null labels");
  const int nc = e.out_c_ - 4, nb = e.out_h_ * e.out_w_;
  det_begin("vp_metric_add_det", nc, nb, n_labels, iou_v, n_iou, conf, iou);
  const float* d_labels = n_labels > 0 ? static_cast<const float*>(stage_host(det_stage_, labels, sizeof(float) * 5 * (size_t)n_labels)) : nullptr;
  wait_for(e, ev_src_[0]);
  det_chain(e.d_logits_, nc, nb, conf, iou, 0);
  release_to(e, ev_read_[0]);
  det_match(d_labels, nullptr, n_labels, 0, e.net_h(), e.net_w());
}

void Metric::add_det_pair(Engine& e, Engine& ref, float label_conf, float conf, float iou, const float* iou_v, int n_iou) {
  det_source_of(e, "vp_metric_add_det_pair");
  det_source_of(ref, "vp_metric_add_det_pair");
  if (e.out_c_ != ref.out_c_ || e.out_h_ * e.out_w_ != ref.out_h_ * ref.out_w_) throw std::invalid_argument("vp_metric_add_det_pair: the two engines differ in nc or nb");
  if (label_conf != label_conf) throw std::invalid_argument("vp_metric_add_det_pair: a NaN threshold");
  const int nc = e.out_c_ - 4, nb = e.out_h_ * e.out_w_;
  det_begin("vp_metric_add_det_pair", nc, nb, kDetValMaxDet, iou_v, n_iou, conf, iou);
  wait_for(e, ev_src_[0]);
  if (&ref != &e) wait_for(ref, ev_src_[1]);
  const DetValParams r = det_chain(ref.d_logits_, nc, nb, conf, iou, 1);
  DetValLabelsParams lp{};
  lp.rows = r.rows;
  lp.counts = r.counts;
  lp.label_conf = label_conf;
  lp.labels = reinterpret_cast<float*>(d_det_small_ + kDetSmallLabels);
  lp.n_labels = reinterpret_cast<unsigned*>(d_det_small_ + kDetSmallLabels + 6144);
  VP_HIP_CHECK(launch_det_val_labels(lp, stream_));
  det_chain(e.d_logits_, nc, nb, conf, iou, 0);
  release_to(e, ev_read_[0]);
  if (&ref != &e) release_to(ref, ev_read_[1]);
  det_match(lp.labels, lp.n_labels, kDetValMaxDet, 1, e.net_h(), e.net_w());
}

void Metric::add_det_raw(const float* raw, bool on_device, int nc, int nb, int net_h, int net_w, const float* labels, int n_labels, float conf, float iou, const float* iou_v,
                         int n_iou) {
  if (!raw || (n_labels > 0 && !labels)) throw std::invalid_argument("vp_metric_add_det_raw: null tensor or null labels");
  if (net_h < 1 || net_w < 1) throw std::invalid_argument("vp_metric_add_det_raw: net_h, net_w below 1");
  det_begin("vp_metric_add_det_raw", nc, nb, n_labels, iou_v, n_iou, conf, iou);
  const float* d_raw = on_device ? raw : static_cast<const float*>(stage_host(stage_[0], raw, sizeof(float) * (size_t)(4 + nc) * nb));
  if (reinterpret_cast<uintptr_t>(d_raw) & 3) throw std::invalid_argument("vp_metric_add_det_raw: device tensor not aligned to 4 bytes");
  const float* d_labels = n_labels > 0 ? static_cast<const float*>(stage_host(det_stage_, labels, sizeof(float) * 5 * (size_t)n_labels)) : nullptr;
  det_chain(d_raw, nc, nb, conf, iou, 0);
  det_match(d_labels, nullptr, n_labels, 0, net_h, net_w);
}

void Metric::fetch_det(std::vector<DetFrameRecord>* frames, std::vector<DetRowRecord>* rows, std::vector<float>* label_cls) {
  VP_HIP_CHECK(hipSetDevice(gpu_));
  frames->assign((size_t)det_frames_, DetFrameRecord{});
  rows->clear();
  label_cls->clear();
  unsigned totals[2] = {0, 0};
  if (det_frames_) {
    VP_HIP_CHECK(hipMemcpyAsync(frames->data(), d_det_frames_, (size_t)det_frames_ * sizeof(DetFrameRecord), hipMemcpyDeviceToHost, stream_));
    VP_HIP_CHECK(hipMemcpyAsync(totals, d_det_small_, sizeof(totals), hipMemcpyDeviceToHost, stream_));
  }
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
  rows->assign((size_t)totals[0], DetRowRecord{});
  label_cls->assign((size_t)totals[1], 0.0f);
  if (totals[0]) VP_HIP_CHECK(hipMemcpyAsync(rows->data(), d_det_rows_, (size_t)totals[0] * sizeof(DetRowRecord), hipMemcpyDeviceToHost, stream_));
  if (totals[1]) VP_HIP_CHECK(hipMemcpyAsync(label_cls->data(), d_det_label_cls_, (size_t)totals[1] * sizeof(float), hipMemcpyDeviceToHost, stream_));
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
}

// ---- the lane part: EgoLanes records and AutoSteer line records of their own, allocated by the first add
const Engine& Metric::lanes_source_of(Engine& e, const char* who) const {
  const std::string me(who);
  if (e.gpu_ != gpu_) throw std::invalid_argument(me + ": the engine lives on GPU " + std::to_string(e.gpu_) + ", the metric on GPU " + std::to_string(gpu_));
  if (e.kind_ != 3) throw std::invalid_argument(me + ": VP_EGOLANES engines only (the three lane planes of its logits)");
  if (e.frames_ > 1) throw std::invalid_argument(me + ": a batched encoder has no outputs of its own (score its per-camera heads)");
  if (!e.have_outputs_) throw std::runtime_error("Inference has not been run yet");
  if (!e.d_logits_ || e.out_c_ != 3) throw std::invalid_argument(me + ": the engine has no logits of three planes");
  return e;
}

const Engine& Metric::rows_source_of(Engine& e, const char* who) const {
  const std::string me(who);
  if (e.gpu_ != gpu_) throw std::invalid_argument(me + ": the engine lives on GPU " + std::to_string(e.gpu_) + ", the metric on GPU " + std::to_string(gpu_));
  if (e.kind_ != 6) throw std::invalid_argument(me + ": VP_AUTOSTEER engines only (the lane rows xp / h_vector of its logits)");
  if (!e.have_outputs_) throw std::runtime_error("Inference has not been run yet");
  if (!e.d_logits_ || e.out_c_ != 2 || e.out_w_ != 1 || e.out_h_ < 1 || e.out_h_ > kMetricRowsMaxRows) throw std::invalid_argument(me + ": the engine has no xp / h_vector rows");
  return e;
}

static void metric_check_lanes_args(const char* who, const void* logits, int h, int w, const void* gt, int gt_form) {
  const std::string me(who);
  if (!logits || !gt) throw std::invalid_argument(me + ": null logits or null ground truth");
  if (gt_form < kLanesGtPlanes || gt_form > kLanesGtBits4x) throw std::invalid_argument(me + ": gt_form " + std::to_string(gt_form) + " (VP_LANES_GT_PLANES, VP_LANES_GT_BITS, VP_LANES_GT_BITS_4X)");
  if (h < kMetricLanesMinSide || w < kMetricLanesMinSide)
    throw std::invalid_argument(me + ": planes of " + std::to_string(h) + " x " + std::to_string(w) + " (the four 2x2 pools need 16 x 16 at least)");
  if ((long long)h * w > (long long)kMetricLanesMaxN) throw std::invalid_argument(me + ": h * w above 2^22");
}

static size_t lanes_gt_bytes(int gt_form, int h, int w) {
  const size_t n = (size_t)h * w;
  return gt_form == kLanesGtPlanes ? 3 * sizeof(float) * n : (gt_form == kLanesGtBits ? n : 16 * n);
}

LanesRecord* Metric::lanes_next(const char* who) {
  if (lanes_frames_ >= max_frames_)
    throw std::runtime_error(std::string(who) + ": the lanes accumulator is full (" + std::to_string(max_frames_) + " frames; vp_metric_fetch_lanes, then vp_metric_reset)");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  if (!d_lanes_records_) VP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_lanes_records_), (size_t)max_frames_ * sizeof(LanesRecord)));
  return d_lanes_records_ + lanes_frames_;
}

// scratch: the partials [3][7][kMetricBlocks] doubles, then (h * w above kMetricLanesLdsN) D0 [3][n] and the pooled levels [3][metric_lanes_pooled_elems]
void Metric::lanes(const float* d_logits, const void* d_gt, int gt_form, int h, int w, LanesRecord* rec) {
  const size_t n = (size_t)h * w, pe = metric_lanes_pooled_elems(h, w);
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const bool general = n > kMetricLanesLdsN;
  const size_t o_d0 = up(3 * 7 * kMetricBlocks * sizeof(double)), o_pool = o_d0 + (general ? up(12 * n) : 0), total = o_pool + (general ? up(12 * pe) : 0);
  grow(d_lanes_scratch_, lanes_scratch_cap_, total);
  if ((reinterpret_cast<uintptr_t>(d_logits) & 3) || (gt_form != kLanesGtBits && (reinterpret_cast<uintptr_t>(d_gt) & 3)))
    throw std::invalid_argument("vp_metric lanes: device logits or ground truth not aligned to 4 bytes");
  MetricLanesParams q{};
  q.logits = d_logits;
  q.gt = d_gt;
  q.gt_form = gt_form;
  q.h = h;
  q.w = w;
  q.part = reinterpret_cast<double*>(d_lanes_scratch_);
  q.d0 = general ? reinterpret_cast<float*>(d_lanes_scratch_ + o_d0) : nullptr;
  q.pooled = general ? reinterpret_cast<float*>(d_lanes_scratch_ + o_pool) : nullptr;
  q.rec = rec;
  VP_HIP_CHECK(launch_metric_lanes(q, stream_));
}

void Metric::add_lanes(Engine& e, const void* gt, bool gt_on_device, int gt_form) {
  lanes_source_of(e, "vp_metric_add_lanes");
  metric_check_lanes_args("vp_metric_add_lanes", e.d_logits_, e.out_h_, e.out_w_, gt, gt_form);
  LanesRecord* rec = lanes_next("vp_metric_add_lanes");
  const void* d_gt = gt_on_device ? gt : stage_host(stage_[1], gt, lanes_gt_bytes(gt_form, e.out_h_, e.out_w_));
  wait_for(e, ev_src_[0]);
  lanes(e.d_logits_, d_gt, gt_form, e.out_h_, e.out_w_, rec);
  release_to(e, ev_read_[0]);
  ++lanes_frames_;
}

void Metric::add_lanes_pair(Engine& e, Engine& ref) {
  lanes_source_of(e, "vp_metric_add_lanes_pair");
  lanes_source_of(ref, "vp_metric_add_lanes_pair");
  if (e.out_h_ != ref.out_h_ || e.out_w_ != ref.out_w_) throw std::invalid_argument("vp_metric_add_lanes_pair: the two engines are of different output sizes");
  metric_check_lanes_args("vp_metric_add_lanes_pair", e.d_logits_, e.out_h_, e.out_w_, ref.d_logits_, kLanesGtPlanes);
  LanesRecord* rec = lanes_next("vp_metric_add_lanes_pair");
  wait_for(e, ev_src_[0]);
  if (&ref != &e) wait_for(ref, ev_src_[1]);
  lanes(e.d_logits_, ref.d_logits_, kLanesGtRef, e.out_h_, e.out_w_, rec);
  release_to(e, ev_read_[0]);
  if (&ref != &e) release_to(ref, ev_read_[1]);
  ++lanes_frames_;
}

void Metric::add_lanes_logits(const float* logits, bool on_device, int h, int w, const void* gt, bool gt_on_device, int gt_form) {
  metric_check_lanes_args("vp_metric_add_lanes_logits", logits, h, w, gt, gt_form);
  LanesRecord* rec = lanes_next("vp_metric_add_lanes_logits");
  const float* d_logits = on_device ? logits : static_cast<const float*>(stage_host(stage_[0], logits, 3 * sizeof(float) * (size_t)h * w));
  const void* d_gt = gt_on_device ? gt : stage_host(stage_[1], gt, lanes_gt_bytes(gt_form, h, w));
  lanes(d_logits, d_gt, gt_form, h, w, rec);
  ++lanes_frames_;
}

void Metric::fetch_lanes(LanesRecord* out, int count) {
  if (count < 0 || count > lanes_frames_ || (count > 0 && !out)) throw std::invalid_argument("vp_metric_fetch_lanes: more records than were added, or a null buffer");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  if (count) VP_HIP_CHECK(hipMemcpyAsync(out, d_lanes_records_, (size_t)count * sizeof(LanesRecord), hipMemcpyDeviceToHost, stream_));
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
}

RowsRecord* Metric::rows_next(const char* who, int n_lines, const double* thr, int n_thr) {
  const std::string me(who);
  if (!thr || n_thr < 1 || n_thr > kMetricRowsMaxThr) throw std::invalid_argument(me + ": a null threshold table, or n_thr outside 1 .. 8");
  for (int k = 0; k < n_thr; ++k)
    if (thr[k] != thr[k]) throw std::invalid_argument(me + ": a NaN threshold");
  if (rows_lines_ && (n_thr != rows_n_thr_ || std::memcmp(thr, rows_thr_, sizeof(double) * (size_t)n_thr) != 0))
    throw std::invalid_argument(me + ": another threshold table than the lines added so far were scored with (vp_metric_reset first)");
  if (rows_lines_ + n_lines > max_frames_)
    throw std::runtime_error(me + ": the rows accumulator is full (" + std::to_string(max_frames_) + " lines; vp_metric_fetch_rows, then vp_metric_reset)");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  if (!d_rows_records_) VP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_rows_records_), (size_t)max_frames_ * sizeof(RowsRecord)));
  rows_n_thr_ = n_thr;
  std::memcpy(rows_thr_, thr, sizeof(double) * (size_t)n_thr);
  return d_rows_records_ + rows_lines_;
}

void Metric::rows(const float* xp, const float* hv, const float* txp, const float* thv, int n_lines, int n_rows, RowsRecord* rec) {
  MetricRowsParams q{};
  q.xp = xp;
  q.hv = hv;
  q.txp = txp;
  q.thv = thv;
  q.n_lines = n_lines;
  q.rows = n_rows;
  q.n_thr = rows_n_thr_;
  std::memcpy(q.thr, rows_thr_, sizeof(q.thr));
  q.rec = rec;
  VP_HIP_CHECK(launch_metric_rows(q, stream_));
  rows_lines_ += n_lines;
}

// the engine's logits {1, 2, rows, 1}: xp, then h_vector
void Metric::add_rows(Engine& e, const float* target_xp, const float* target_h, const double* thr, int n_thr) {
  rows_source_of(e, "vp_metric_add_rows");
  if (!target_xp || !target_h) throw std::invalid_argument("vp_metric_add_rows: null targets");
  RowsRecord* rec = rows_next("vp_metric_add_rows", 1, thr, n_thr);
  const int n = e.out_h_;
  std::vector<float> both(2 * (size_t)n);
  std::memcpy(both.data(), target_xp, sizeof(float) * (size_t)n);
  std::memcpy(both.data() + n, target_h, sizeof(float) * (size_t)n);
  const float* d_t = static_cast<const float*>(stage_host(stage_[1], both.data(), sizeof(float) * both.size()));
  wait_for(e, ev_src_[0]);
  rows(e.d_logits_, e.d_logits_ + n, d_t, d_t + n, 1, n, rec);
  release_to(e, ev_read_[0]);
}

void Metric::add_rows_pair(Engine& e, Engine& ref, const double* thr, int n_thr) {
  rows_source_of(e, "vp_metric_add_rows_pair");
  rows_source_of(ref, "vp_metric_add_rows_pair");
  if (e.out_h_ != ref.out_h_) throw std::invalid_argument("vp_metric_add_rows_pair: the two engines differ in their rows");
  RowsRecord* rec = rows_next("vp_metric_add_rows_pair", 1, thr, n_thr);
  const int n = e.out_h_;
  wait_for(e, ev_src_[0]);
  if (&ref != &e) wait_for(ref, ev_src_[1]);
  rows(e.d_logits_, e.d_logits_ + n, ref.d_logits_, ref.d_logits_ + n, 1, n, rec);
  release_to(e, ev_read_[0]);
  if (&ref != &e) release_to(ref, ev_read_[1]);
}

void Metric::add_rows_raw(const float* xp, const float* hv, const float* target_xp, const float* target_h, int n_lines, int n_rows, const double* thr, int n_thr) {
  if (!xp || !hv || !target_xp || !target_h) throw std::invalid_argument("vp_metric_add_rows_raw: a null array");
  if (n_lines < 1 || n_lines > kMetricRowsMaxLines || n_rows < 1 || n_rows > kMetricRowsMaxRows)
    throw std::invalid_argument("vp_metric_add_rows_raw: n_lines " + std::to_string(n_lines) + ", rows " + std::to_string(n_rows) + " (n_lines 1 .. 8, rows 1 .. 1024)");
  RowsRecord* rec = rows_next("vp_metric_add_rows_raw", n_lines, thr, n_thr);
  const size_t n = (size_t)n_lines * n_rows;
  std::vector<float> all(4 * n);
  const float* src[4] = {xp, hv, target_xp, target_h};
  for (int k = 0; k < 4; ++k) std::memcpy(all.data() + k * n, src[k], sizeof(float) * n);
  const float* d = static_cast<const float*>(stage_host(stage_[0], all.data(), sizeof(float) * all.size()));
  rows(d, d + n, d + 2 * n, d + 3 * n, n_lines, n_rows, rec);
}

void Metric::fetch_rows(RowsRecord* out, int count) {
  if (count < 0 || count > rows_lines_ || (count > 0 && !out)) throw std::invalid_argument("vp_metric_fetch_rows: more records than were added, or a null buffer");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  if (count) VP_HIP_CHECK(hipMemcpyAsync(out, d_rows_records_, (size_t)count * sizeof(RowsRecord), hipMemcpyDeviceToHost, stream_));
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
}

// ---- the label part: ground truth from a label file's decoded pixels, records of their own
void label_nearest_tab(int src, int dst, int* tab) { nearest_tab(src, dst, tab); }

LabelSegParams label_seg_params(const char* who, const void* label, int channels, int h, int w, int stride, const int* crop, const uint8_t* colours, int n_colours) {
  const std::string me(who);
  if (!label) throw std::invalid_argument(me + ": null label");
  if (channels != 1 && channels != 3) throw std::invalid_argument(me + ": channels " + std::to_string(channels) + " (1: a mask label, 3: a colour label)");
  if (h < 1 || w < 1 || h > kLabelMaxSide || w > kLabelMaxSide) throw std::invalid_argument(me + ": a label of " + std::to_string(h) + " x " + std::to_string(w) + " (1 .. 16384 each)");
  if ((long long)stride < (long long)w * channels) throw std::invalid_argument(me + ": stride " + std::to_string(stride) + " below the row's " + std::to_string(w * channels) + " bytes");
  LabelSegParams q{};
  q.channels = channels;
  q.h = h;
  q.w = w;
  q.stride = stride;
  q.cw = w;
  q.ch = h;
  if (crop) {
    for (int k = 0; k < 4; ++k)
      if (crop[k] < kLabelCropMin || crop[k] > kLabelCropMax) throw std::invalid_argument(me + ": a crop coordinate outside -16384 .. 32768");
    q.l = crop[0];
    q.t = crop[1];
    q.cw = crop[2] - crop[0];
    q.ch = crop[3] - crop[1];
    if (q.cw < 1 || q.ch < 1) throw std::invalid_argument(me + ": a crop of " + std::to_string(q.ch) + " x " + std::to_string(q.cw) + " pixels");
  }
  if (channels == 3) {
    if (!colours || n_colours < 1 || n_colours > kLabelMaxColours) throw std::invalid_argument(me + ": a null colour table, or n_colours outside 1 .. 16");
    for (int k = 0; k < n_colours; ++k) {
      if (colours[4 * k + 3] > 2) throw std::invalid_argument(me + ": class " + std::to_string(colours[4 * k + 3]) + " in the colour table (0 .. 2)");
      q.rgb[k] = (unsigned)colours[4 * k] | (unsigned)colours[4 * k + 1] << 8 | (unsigned)colours[4 * k + 2] << 16;
      q.cls[k] = colours[4 * k + 3];
    }
    q.n_colours = n_colours;
  }
  return q;
}

void label_check_depth(const char* who, const void* label, int dtype, int h, int w, int stride) {
  const std::string me(who);
  if (!label) throw std::invalid_argument(me + ": null label");
  if (dtype != kLabelF32 && dtype != kLabelF64) throw std::invalid_argument(me + ": dtype " + std::to_string(dtype) + " (VP_LABEL_F32, VP_LABEL_F64)");
  if (h < 1 || w < 1 || h > kLabelMaxSide || w > kLabelMaxSide) throw std::invalid_argument(me + ": a label of " + std::to_string(h) + " x " + std::to_string(w) + " (1 .. 16384 each)");
  if (stride < w) throw std::invalid_argument(me + ": stride " + std::to_string(stride) + " below the row's " + std::to_string(w) + " elements");
}

// Canvas::table's scheme: the first use of a size uploads its table and waits; the one unused longest goes when there are 16
const int* Metric::label_tab(int src, int dst) {
  for (size_t i = 0; i < label_tabs_.size(); ++i)
    if (label_tabs_[i].src == src && label_tabs_[i].dst == dst) {
      std::rotate(label_tabs_.begin() + i, label_tabs_.begin() + i + 1, label_tabs_.end());
      return label_tabs_.back().idx;
    }
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
  if (label_tabs_.size() >= 16) {
    (void)hipFree(label_tabs_.front().idx);
    label_tabs_.erase(label_tabs_.begin());
  }
  std::vector<int> idx((size_t)dst);
  nearest_tab(src, dst, idx.data());
  LabelTab t{src, dst, nullptr};
  VP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&t.idx), idx.size() * sizeof(int)));
  label_tabs_.push_back(t);   // owned from here on
  VP_HIP_CHECK(hipMemcpyAsync(t.idx, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
  return t.idx;
}

LabelRecord* Metric::label_next(const char* who) {
  if (label_frames_ >= max_frames_)
    throw std::runtime_error(std::string(who) + ": the label accumulator is full (" + std::to_string(max_frames_) + " frames; vp_metric_fetch_labels, then vp_metric_reset)");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  if (!d_label_records_) VP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_label_records_), (size_t)max_frames_ * sizeof(LabelRecord)));
  return d_label_records_ + label_frames_;
}

// scratch: the ground truth [oh][ow] (bytes, or fp32 for a depth label), then the partials.  Everything that may wait (tables, scratch) comes before the copy.
const uint8_t* Metric::label_seg(LabelSegParams q, const uint8_t* label, int oh, int ow, LabelRecord* rec) {
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t o_part = up((size_t)oh * ow);
  q.ty = label_tab(q.ch, oh);
  q.tx = label_tab(q.cw, ow);
  grow(d_label_scratch_, label_scratch_cap_, o_part + up(4 * kMetricBlocks * sizeof(unsigned)));
  q.label = static_cast<const uint8_t*>(stage_host(stage_[1], label, (size_t)(q.h - 1) * q.stride + (size_t)q.w * q.channels));
  q.oh = oh;
  q.ow = ow;
  q.gt = d_label_scratch_;
  q.part = reinterpret_cast<unsigned*>(d_label_scratch_ + o_part);
  q.rec = rec;
  VP_HIP_CHECK(launch_label_seg(q, stream_));
  return q.gt;
}

const float* Metric::label_depth(const void* label, int dtype, int h, int w, int stride, int oh, int ow, LabelRecord* rec) {
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t o_part = up(sizeof(float) * (size_t)oh * ow), es = dtype == kLabelF64 ? sizeof(double) : sizeof(float);
  LabelDepthParams q{};
  q.ty = label_tab(h, oh);
  q.tx = label_tab(w, ow);
  grow(d_label_scratch_, label_scratch_cap_, o_part + up(kMetricBlocks * sizeof(LabelExtPartial)));
  q.label = stage_host(stage_[1], label, es * ((size_t)(h - 1) * stride + (size_t)w));
  q.dtype = dtype;
  q.h = h;
  q.w = w;
  q.stride = stride;
  q.oh = oh;
  q.ow = ow;
  q.gt = reinterpret_cast<float*>(d_label_scratch_);
  q.part = reinterpret_cast<LabelExtPartial*>(d_label_scratch_ + o_part);
  q.rec = rec;
  VP_HIP_CHECK(launch_label_depth(q, stream_));
  return q.gt;
}

void Metric::add_seg_label(Engine& e, const uint8_t* label, int channels, int h, int w, int stride, const int* crop, const uint8_t* colours, int n_colours) {
  source_of(e, "vp_metric_add_seg_label", false);
  const LabelSegParams q = label_seg_params("vp_metric_add_seg_label", label, channels, h, w, stride, crop, colours, n_colours);
  metric_check_seg_args("vp_metric_add_seg_label", e.d_logits_, e.out_c_, e.out_h_, e.out_w_, label, 0);
  MetricRecord* rec = next_record("vp_metric_add_seg_label");
  LabelRecord* lrec = label_next("vp_metric_add_seg_label");
  const uint8_t* d_gt = label_seg(q, label, e.out_h_, e.out_w_, lrec);   // ahead of the wait: the label kernels overlap the engine's pass
  wait_for(e, ev_src_[0]);
  seg(e.d_logits_, nullptr, d_gt, e.out_c_, e.out_h_, e.out_w_, 0, rec);
  release_to(e, ev_read_[0]);
  ++frames_;
  ++label_frames_;
}

void Metric::add_depth_label(Engine& e, const void* label, int dtype, int h, int w, int stride) {
  source_of(e, "vp_metric_add_depth_label", true);
  label_check_depth("vp_metric_add_depth_label", label, dtype, h, w, stride);
  metric_check_depth_args("vp_metric_add_depth_label", e.d_logits_, label, e.out_h_, e.out_w_);
  MetricRecord* rec = next_record("vp_metric_add_depth_label");
  LabelRecord* lrec = label_next("vp_metric_add_depth_label");
  const float* d_gt = label_depth(label, dtype, h, w, stride, e.out_h_, e.out_w_, lrec);
  wait_for(e, ev_src_[0]);
  depth(e.d_logits_, d_gt, e.out_h_, e.out_w_, rec);
  release_to(e, ev_read_[0]);
  ++frames_;
  ++label_frames_;
}

void Metric::add_seg_logits_label(const float* logits, bool on_device, int c, int oh, int ow, const uint8_t* label, int channels, int h, int w, int stride, const int* crop,
                                  const uint8_t* colours, int n_colours) {
  const LabelSegParams q = label_seg_params("vp_metric_add_seg_logits_label", label, channels, h, w, stride, crop, colours, n_colours);
  metric_check_seg_args("vp_metric_add_seg_logits_label", logits, c, oh, ow, label, 0);
  if (on_device && (reinterpret_cast<uintptr_t>(logits) & 3)) throw std::invalid_argument("vp_metric_add_seg_logits_label: device logits not aligned to 4 bytes");
  MetricRecord* rec = next_record("vp_metric_add_seg_logits_label");
  LabelRecord* lrec = label_next("vp_metric_add_seg_logits_label");
  const float* d_logits = on_device ? logits : static_cast<const float*>(stage_host(stage_[0], logits, sizeof(float) * (size_t)oh * ow * c));
  const uint8_t* d_gt = label_seg(q, label, oh, ow, lrec);
  seg(d_logits, nullptr, d_gt, c, oh, ow, 0, rec);
  ++frames_;
  ++label_frames_;
}

void Metric::add_depth_plane_label(const float* pred, bool pred_on_device, int oh, int ow, const void* label, int dtype, int h, int w, int stride) {
  label_check_depth("vp_metric_add_depth_plane_label", label, dtype, h, w, stride);
  metric_check_depth_args("vp_metric_add_depth_plane_label", pred, label, oh, ow);
  if (pred_on_device && (reinterpret_cast<uintptr_t>(pred) & 3)) throw std::invalid_argument("vp_metric_add_depth_plane_label: device plane not aligned to 4 bytes");
  MetricRecord* rec = next_record("vp_metric_add_depth_plane_label");
  LabelRecord* lrec = label_next("vp_metric_add_depth_plane_label");
  const float* d_pred = pred_on_device ? pred : static_cast<const float*>(stage_host(stage_[0], pred, sizeof(float) * (size_t)oh * ow));
  const float* d_gt = label_depth(label, dtype, h, w, stride, oh, ow, lrec);
  depth(d_pred, d_gt, oh, ow, rec);
  ++frames_;
  ++label_frames_;
}

void Metric::fetch_labels(LabelRecord* out, int count) {
  if (count < 0 || count > label_frames_ || (count > 0 && !out)) throw std::invalid_argument("vp_metric_fetch_labels: more records than were added, or a null buffer");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  if (count) VP_HIP_CHECK(hipMemcpyAsync(out, d_label_records_, (size_t)count * sizeof(LabelRecord), hipMemcpyDeviceToHost, stream_));
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
}

// -------------------------------------------------------------------------------------------------- timing
void Engine::timer_begin() { VP_HIP_CHECK(hipEventRecord(ev0_, stream_)); }
float Engine::timer_end() {
  VP_HIP_CHECK(hipEventRecord(ev1_, stream_));
  VP_HIP_CHECK(hipEventSynchronize(ev1_));
  float ms = 0.f;
  VP_HIP_CHECK(hipEventElapsedTime(&ms, ev0_, ev1_));
  return ms;
}

int Engine::profile_layers(int iters, float* ms, int cap) {
  const size_t first = input_is_tensor_ ? first_net_op_ : 0;
  const int n = (int)ops_.size();
  if (cap < n) throw std::invalid_argument("profile buffer too small");
  if (base_) {
    if (!base_->have_outputs_) throw std::runtime_error("shared engine: run the base engine on a frame first");
  } else if (!input_is_tensor_ && !d_frame_) {
    throw std::runtime_error("no frame resident");
  }
  std::vector<hipEvent_t> ev(n + 1);
  for (auto& e : ev) VP_HIP_CHECK(hipEventCreate(&e));
  std::vector<double> acc(n, 0.0);
  for (int it = 0; it < iters + 1; ++it) {  // iteration 0 is a warm-up
    for (int i = (int)first; i < n; ++i) {
      VP_HIP_CHECK(hipEventRecord(ev[i], stream_));
      hipError_t e = ops_[i].run(stream_);
      if (e != hipSuccess) throw std::runtime_error("launch failed in layer '" + ops_[i].name + "'");
    }
    VP_HIP_CHECK(hipEventRecord(ev[n], stream_));
    VP_HIP_CHECK(hipStreamSynchronize(stream_));
    if (it == 0) continue;
    for (int i = (int)first; i < n; ++i) {
      float t = 0.f;
      VP_HIP_CHECK(hipEventElapsedTime(&t, ev[i], ev[i + 1]));
      acc[i] += t;
    }
  }
  for (int i = 0; i < n; ++i) ms[i] = (float)(acc[i] / std::max(1, iters));
  for (auto& e : ev) hipEventDestroy(e);
  warmed_ = true;
  have_outputs_ = true;
  return n;
}

void Engine::read_act(int i, float* dst) {
  if (i < 0 || i >= (int)acts_.size()) throw std::invalid_argument("tensor index out of range");
  const Act& a = *acts_[i];
  const size_t n = (size_t)a.Creal * a.H * a.W;
  float* d = nullptr;
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
  VP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d), n * sizeof(float)));
  hipError_t e = launch_act_to_nchw(a.view(), a.Creal, d, stream_, act_mul(&a));   // true values (VP_ACT_SCALE: times 2^s of the tensor)
  if (e == hipSuccess) e = hipStreamSynchronize(stream_);
  if (e == hipSuccess) e = hipMemcpyAsync(dst, d, n * sizeof(float), hipMemcpyDeviceToHost, stream_);   // (not the legacy stream: engine.hpp copy_h2d)
  if (e == hipSuccess) e = hipStreamSynchronize(stream_);
  hipFree(d);
  VP_HIP_CHECK(e);
}

// ------------------------------------------------------------------------------------------------ VP_ACT_SCALE
// Per-tensor power-of-two activation scale (DESIGN.md section 4 "Range").  A flagged engine stores tensor t as x * 2^-s_t; the exponents live in
// act_exp_ (one per TIE GROUP: tensors that share storage or are copies / max-pools of each other), every launch reads them when it runs.
void Engine::tie_acts(const Act* a, const Act* b) {
  if (!act_scale() || !a || !b || a->tie == b->tie) return;
  const int from = b->tie, to = a->tie;
  if (act_exp_[from] != act_exp_[to]) throw std::invalid_argument("tied tensors carry different exponents: " + a->name + ", " + b->name);
  for (auto& t : acts_)
    if (t->tie == from) t->tie = to;
}

void Engine::set_act_exp(const Act* a, int e) {
  if (!act_scale() || !a || a->tie < 0) throw std::invalid_argument("VP_ACT_SCALE: not a tensor of a flagged engine");
  if (e < -60 || e > 60) throw std::invalid_argument("VP_ACT_SCALE: exponent out of range (-60 .. 60)");
  act_exp_[a->tie] = e;
  exps_changed();
}

std::vector<int> Engine::act_scales() const {
  std::vector<int> v(acts_.size(), 0);
  for (size_t i = 0; i < acts_.size(); ++i) v[i] = act_exp(acts_[i].get());
  return v;
}

void Engine::set_act_scales(const int* exps, int n) {
  if (!act_scale()) throw std::invalid_argument("vp_set_act_scales: the engine was not created with VP_ACT_SCALE");
  if (!exps || n != (int)acts_.size()) throw std::invalid_argument("vp_set_act_scales: the table needs one exponent per tensor (" + std::to_string(acts_.size()) + ")");
  std::vector<int> grp(act_exp_.size(), INT_MIN);
  for (int i = 0; i < n; ++i) {
    const Act& a = *acts_[i];
    if (exps[i] < -60 || exps[i] > 60) throw std::invalid_argument("vp_set_act_scales: exponent out of range (-60 .. 60): " + a.name);
    if (grp[a.tie] != INT_MIN && grp[a.tie] != exps[i]) throw std::invalid_argument("vp_set_act_scales: tied tensors disagree at '" + a.name + "' (tensors that share storage share one exponent)");
    grp[a.tie] = exps[i];
  }
  for (size_t g = 0; g < grp.size(); ++g)
    if (grp[g] != INT_MIN) {
      act_exp_[g] = grp[g];
      act_exp_seen_[g] = 1;   // an installed exponent counts as measured: a later calibration only raises it
    }
  ad_primed_ = false;   // features parked under the old exponents are not carried over
  exps_changed();
}

void Engine::reset_range() {
  if (!act_scale()) throw std::invalid_argument("vp_reset_range: the engine was not created with VP_ACT_SCALE");
  std::fill(act_exp_.begin(), act_exp_.end(), 0);
  std::fill(act_exp_seen_.begin(), act_exp_seen_.end(), 0);
  ad_primed_ = false;
  exps_changed();
}

void Engine::stash_previous_frame() {
  if (!act_scale() || !d_frame_ || input_is_tensor_) return;
  const size_t need = (size_t)frame_h_ * frame_stride_;
  if (need > prev_frame_cap_) {
    VP_HIP_CHECK(hipStreamSynchronize(stream_));
    if (d_prev_frame_) dfree(d_prev_frame_);
    d_prev_frame_ = static_cast<uint8_t*>(dalloc(std::max(need, frame_cap_), false));
    prev_frame_cap_ = std::max(need, frame_cap_);
  }
  VP_HIP_CHECK(hipMemcpyAsync(d_prev_frame_, d_frame_, need, hipMemcpyDeviceToDevice, stream_));
  prev_frame_stashed_ = true;   // upload_frame turns it into prev_frame_valid_ for the ONE frame uploaded next (the pair's current half)
}

// The eager walk of the plan that calibration and the range survey share: launch by launch on the resident input (the uploaded frame, or the tensor
// vp_infer_tensor / vp_detect_infer left), `visit` behind every launch for every tensor the launch stores (Op::writes).  AutoDrive pairs the resident frame
// with the previous one (head.cat carries both): a round is a features-only pass over the previous frame (`prime`: up to the launch that parks P5, the
// shift left out) -- the stashed frame of vp_infer_pair where the engine keeps one, else the resident frame again -- and then the whole plan on the current
// one.  The detector and the lane network are single-frame plans like the scene networks: one pass, and the AutoDrive-only launch indices stay out of it.
// A visitor that returns false starts the round over (at most 16 rounds).
bool Engine::walk_stored(const StoredVisitor& visit) {
  const size_t first = input_is_tensor_ ? first_net_op_ : 0;
  const bool ad = kind_ == 4;
  const size_t shift_op = ad ? ad_shift_op_ : SIZE_MAX;
  auto pass = [&](size_t begin, size_t end, bool prime) -> bool {
    for (size_t i = begin; i < end; ++i) {
      if (prime && i == shift_op) continue;
      run_ops(stream_, i, i + 1);
      for (const Act* a : ops_[i].writes)
        if (!visit(i, a, begin, prime)) return false;
    }
    return true;
  };
  if (!ad) return pass(first, ops_.size(), false);
  const bool pair = prev_frame_valid_ && !input_is_tensor_ && prev_frame_cap_ >= (size_t)frame_h_ * frame_stride_;
  bool done = false;
  for (int round = 0; round < 16 && !done; ++round) {
    if (pair) std::swap(d_frame_, d_prev_frame_);
    try {
      pass(first, ad_place_op_ + 1, true);   // the previous frame (or the resident one again): features only
    } catch (...) {
      if (pair) std::swap(d_frame_, d_prev_frame_);
      throw;
    }
    if (pair) std::swap(d_frame_, d_prev_frame_);
    done = pass(first, ops_.size(), false);
  }
  return done;
}

// Runs the plan eagerly (walk_stored), measures every tensor a launch stores (act_absmax_kernel) and moves its exponent so that the stored abs-max lies in
// [2^(target - 1), 2^target).  The first measurement of a tensor since vp_reset_range sets the exponent, later ones only raise it: calibrating on several
// frames gives the per-tensor maximum.
void Engine::calibrate_range(int target_log2) {
  if (!act_scale() || (kind_ != 4 && kind_ != 5 && kind_ != 6)) throw std::invalid_argument("vp_calibrate_range: engines created with VP_ACT_SCALE only");
  if (target_log2 == 0) target_log2 = 12;
  if (target_log2 < 1 || target_log2 > 15) throw std::invalid_argument("vp_calibrate_range: target_log2 is 1 .. 15 (0 = the default, 12)");
  if (!input_is_tensor_ && !d_frame_) throw std::runtime_error("no frame resident: call vp_upload_frame / vp_infer_pair first");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
  if (!d_absmax_) d_absmax_ = static_cast<unsigned*>(dalloc(2 * sizeof(unsigned)));
  const bool ad = kind_ == 4;
  const size_t shift_op = ad ? ad_shift_op_ : SIZE_MAX;
  const int head_tie = (!ad || ops_[ad_place_op_].writes.empty()) ? -1 : ops_[ad_place_op_].writes[0]->tie;
  std::vector<int> raises(act_exp_.size(), 0), lower(act_exp_.size(), INT_MIN);
  for (size_t g = 0; g < lower.size(); ++g)
    if (act_exp_seen_[g]) lower[g] = act_exp_[g];
  // false: the exponent of the tensor that carries the previous frame's features (head.cat) moved behind the shift -- the round starts over
  auto settle = [&](size_t i, const Act* a, size_t begin, bool prime) -> bool {
    const int g = a->tie;
    if (g < 0) return true;
    bool restart = false;
    for (;;) {
      unsigned r[2] = {0u, 0u};
      fill_zero(d_absmax_, sizeof(r));
      VP_HIP_CHECK(launch_act_absmax(a->hi, a->lo, a->Creal, a->H, a->W, a->C, d_absmax_, stream_));
      copy_d2h(r, d_absmax_, sizeof(r));
      float amax;
      std::memcpy(&amax, &r[0], sizeof(float));
      const bool bad = r[1] != 0u;
      int want = act_exp_[g];
      if (bad) {
        if (++raises[g] > 3) throw RangeError("vp_calibrate_range: tensor '" + a->name + "' still holds non-finite values after its exponent was raised 3 times by 16");
        want += 16;
      } else if (amax == 0.0f) {
        break;   // an all-zero tensor keeps its exponent
      } else {
        int e2 = 0;
        std::frexp(amax, &e2);   // stored abs-max in [2^(e2 - 1), 2^e2)
        want = std::max(lower[g], act_exp_[g] + e2 - target_log2);
        lower[g] = want;
        act_exp_seen_[g] = 1;
      }
      if (want == act_exp_[g]) break;
      act_exp_[g] = want;
      // head.cat also holds the PREVIOUS frame's features, stored under the old exponent: settle the exponent on this frame first (so that the
      // previous frame's smaller values cannot take it back), then start the round over
      if (ad && !prime && g == head_tie && i >= shift_op) restart = true;
      for (size_t j = begin; j <= i; ++j) {   // every launch so far that writes the tensor stores it again
        if (j == shift_op) continue;
        bool writes = false;
        for (const Act* w : ops_[j].writes) writes |= w->tie == g;
        if (writes) run_ops(stream_, j, j + 1);
      }
      if (!bad) break;
    }
    return !restart;
  };
  bool done = false;
  try {
    done = walk_stored(settle);
  } catch (...) {
    hipStreamSynchronize(stream_);
    ad_primed_ = false;
    exps_changed();
    throw;
  }
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
  ad_primed_ = ad && done;   // the current frame's features sit in the "current" slot under the final exponents
  exps_changed();
  if (!done) throw RangeError("vp_calibrate_range: the exponents did not settle");
}

// ------------------------------------------------------------------------------------------------ VP_MFMA_FP8
// Per-layer activation exponents of the e4m3 MFMA layers (include/vp_hip.h "FP8 MFMA ENGINES").  The launches read f8_layers_[..].qexp when they run, so a
// changed exponent only invalidates the captured graph -- the mechanism of VP_ACT_SCALE, per layer instead of per tensor.
void Engine::set_fp8_exps(const int* exps, int n) {
  if (!mfma_fp8()) throw std::invalid_argument("vp_set_fp8_exps: the engine was not created with VP_MFMA_FP8");
  if (!exps || n != (int)f8_layers_.size()) throw std::invalid_argument("vp_set_fp8_exps: the table needs one exponent per fp8 layer (" + std::to_string(f8_layers_.size()) + ")");
  for (int i = 0; i < n; ++i)
    if (exps[i] < -24 || exps[i] > 24) throw std::invalid_argument("vp_set_fp8_exps: exponent out of range (-24 .. 24): " + ops_[f8_layers_[i].op].name);
  for (int i = 0; i < n; ++i) {
    f8_layers_[i].qexp = exps[i];
    f8_layers_[i].seen = true;   // an installed exponent counts as measured: a later calibration only raises it
  }
  exps_changed();
}

void Engine::reset_fp8() {
  if (!mfma_fp8()) throw std::invalid_argument("vp_reset_fp8: the engine was not created with VP_MFMA_FP8");
  for (Fp8Layer& l : f8_layers_) {
    l.qexp = 0;
    l.seen = false;
  }
  exps_changed();
}

// One eager pass over the resident frame (walk_stored).  Behind the launch that stores the input tensor of an fp8 layer the tensor's abs-max is measured
// (act_absmax_kernel) and the layer's qexp set so that absmax * 2^-qexp lies in [2^(target - 1), 2^target) -- before that layer runs, so every layer
// downstream sees what the calibrated layers ahead of it produce.  An all-zero (or all non-finite) tensor leaves qexp as it is; later calls only raise.
void Engine::calibrate_fp8(int target_log2) {
  if (!mfma_fp8()) throw std::invalid_argument("vp_calibrate_fp8: the engine was not created with VP_MFMA_FP8");
  if (target_log2 == 0) target_log2 = 8;
  if (target_log2 < 1 || target_log2 > 8) throw std::invalid_argument("vp_calibrate_fp8: target_log2 is 1 .. 8 (0 = the default, 8: 1.75x headroom below 448)");
  if (!input_is_tensor_ && !d_frame_) throw std::runtime_error("no frame resident: call vp_upload_frame / vp_infer first");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
  if (!d_absmax_) d_absmax_ = static_cast<unsigned*>(dalloc(2 * sizeof(unsigned)));
  auto settle = [&](size_t i, const Act* a, size_t, bool) -> bool {
    for (Fp8Layer& l : f8_layers_) {
      if (l.tensor < 0 || acts_[l.tensor].get() != a || l.op <= i) continue;
      bool last = true;   // the finished tensor: no launch between this one and the layer stores it again
      for (size_t j = i + 1; j < l.op && last; ++j)
        for (const Act* w : ops_[j].writes) last = last && w != a;
      if (!last) continue;
      unsigned r[2] = {0u, 0u};
      fill_zero(d_absmax_, sizeof(r));
      VP_HIP_CHECK(launch_act_absmax(a->hi, a->lo, a->Creal, a->H, a->W, a->C, d_absmax_, stream_));
      copy_d2h(r, d_absmax_, sizeof(r));
      float amax;
      std::memcpy(&amax, &r[0], sizeof(float));
      if (!(amax > 0.0f)) continue;
      int e2 = 0;
      std::frexp(amax, &e2);   // abs-max in [2^(e2 - 1), 2^e2)
      const int want = std::max(-24, std::min(24, e2 - target_log2));
      l.qexp = l.seen ? std::max(l.qexp, want) : want;
      l.seen = true;
    }
    return true;
  };
  try {
    walk_stored(settle);
  } catch (...) {
    hipStreamSynchronize(stream_);
    exps_changed();
    throw;
  }
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
  exps_changed();
}

// vp_range_survey: the same walk with a visitor that only measures.  Behind the LAST launch that stores a tensor (alias slices of a concatenation, in-place
// copies: one measurement of the finished tensor) it queues act_absmax_kernel and act_exp_hist_kernel on the stored planes; nothing is read back until the
// pass has ended, so the survey costs one synchronisation.  No exponent, launch or graph changes: the engine is left as a plain pass over the same input
// leaves it, outputs on the device included.  Non-finite values are what the survey reports, never an error of its own.
std::vector<Engine::RangeStats> Engine::range_survey() {
  if (base_ || frames_ != 1) throw std::invalid_argument("vp_range_survey: the engine must own its whole network (not a shared-prefix head, not a batched encoder)");
  if (!input_is_tensor_ && !d_frame_) throw std::runtime_error("no frame resident: call vp_upload_frame / vp_infer first");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
  constexpr size_t kWords = VP_HIST_WORDS + 1;   // word 0: {abs-max bits, non-finite count} as launch_act_absmax writes them, then the histogram's words
  const size_t n = acts_.size();
  if (!d_survey_) d_survey_ = static_cast<unsigned long long*>(dalloc(n * kWords * sizeof(unsigned long long)));
  fill_zero(d_survey_, n * kWords * sizeof(unsigned long long));
  std::map<const Act*, size_t> index, last;
  for (size_t t = 0; t < n; ++t) index[acts_[t].get()] = t;
  for (size_t i = input_is_tensor_ ? first_net_op_ : 0; i < ops_.size(); ++i)
    for (const Act* a : ops_[i].writes) last[a] = i;
  std::vector<char> measured(n, 0);
  auto measure = [&](size_t i, const Act* a, size_t, bool prime) -> bool {
    const auto it = index.find(a);
    if (prime || it == index.end() || last[a] != i || measured[it->second]) return true;
    unsigned long long* d = d_survey_ + it->second * kWords;
    VP_HIP_CHECK(launch_act_absmax(a->hi, a->lo, a->Creal, a->H, a->W, a->C, reinterpret_cast<unsigned*>(d), stream_));
    VP_HIP_CHECK(launch_act_exp_hist(a->hi, a->lo, a->Creal, a->H, a->W, a->C, d + 1, stream_));
    measured[it->second] = 1;
    return true;
  };
  try {
    walk_stored(measure);
  } catch (...) {
    hipStreamSynchronize(stream_);
    ad_primed_ = false;
    throw;
  }
  std::vector<unsigned long long> host(n * kWords);
  copy_d2h(host.data(), d_survey_, host.size() * sizeof(unsigned long long));
  ad_primed_ = kind_ == 4;   // the current frame's features sit in the "current" slot, as behind any pass
  have_outputs_ = true;
  host_logits_valid_ = host_mask_valid_ = false;
  note_pass();
  std::vector<RangeStats> out(n);
  for (size_t t = 0; t < n; ++t) {
    RangeStats& r = out[t];
    r.exp = act_exp(acts_[t].get());
    if (!measured[t]) continue;
    const unsigned long long* w = host.data() + t * kWords;
    const unsigned amax_bits = (unsigned)(w[0] & 0xFFFFFFFFull);
    std::memcpy(&r.absmax, &amax_bits, sizeof(float));
    r.nonfinite = w[0] >> 32;
    for (int k = 0; k < VP_HIST_BINS; ++k) r.bins[k] = w[1 + k];
    r.zeros = w[1 + VP_HIST_BINS];
    r.count = w[2 + VP_HIST_BINS];
  }
  return out;
}

// -------------------------------------------------------------------------------------------------- vp_lanes
namespace {
using i128 = __int128;
using u128 = unsigned __int128;

// num / den (den != 0) rounded once to the nearest double, ties to even: the quotient's bits are produced by long division until 64 are significant,
// the rest is a sticky bit
double quotient_rn(i128 num, i128 den) {
  if (num == 0) return 0.0;
  const bool neg = (num < 0) != (den < 0);
  const u128 n = num < 0 ? (u128)0 - (u128)num : (u128)num, d = den < 0 ? (u128)0 - (u128)den : (u128)den;   // d < 2^127: the remainder may be doubled
  u128 q = n / d, r = n % d;
  int e = 0;
  bool sticky = false;
  const u128 top = (u128)1 << 63;
  while (q < top) {
    q <<= 1;
    r <<= 1;
    if (r >= d) r -= d, q |= 1;
    --e;
  }
  while (q >= (top << 1)) {
    sticky = sticky || (q & 1);
    q >>= 1;
    ++e;
  }
  sticky = sticky || r != 0;
  const uint64_t q64 = (uint64_t)q, low = q64 & 0x7FFu;
  uint64_t m = q64 >> 11;   // 53 bits
  if (low > 0x400u || (low == 0x400u && (sticky || (m & 1)))) ++m;
  const double v = std::ldexp((double)m, e + 11);
  return neg ? -v : v;
}
}  // namespace

bool lanes_fit(const long long S[5], const long long T[3], int order, double out[3]) {
  if (!S || !T || !out) throw std::invalid_argument("vp_lanes_fit: null moments or null result");
  if (order != 1 && order != 2) throw std::invalid_argument("vp_lanes_fit: order " + std::to_string(order) + " (1: a line, 2: a quadratic)");
  const long long lim = 1ll << 40;
  for (int k = 0; k < 5; ++k)
    if (S[k] <= -lim || S[k] >= lim || (k < 3 && (T[k] <= -lim || T[k] >= lim))) throw std::invalid_argument("vp_lanes_fit: a moment of 2^40 or more");
  const i128 s0 = S[0], s1 = S[1], s2 = S[2], s3 = S[3], s4 = S[4], t0 = T[0], t1 = T[1], t2 = T[2];
  if (order == 1) {   // [s2 s1; s1 s0] (b, c) = (t1, t0)
    const i128 det = s2 * s0 - s1 * s1;
    if (det == 0) return false;
    out[0] = 0.0;
    out[1] = quotient_rn(t1 * s0 - t0 * s1, det);
    out[2] = quotient_rn(s2 * t0 - s1 * t1, det);
    return true;
  }
  // [s4 s3 s2; s3 s2 s1; s2 s1 s0] (a, b, c) = (t2, t1, t0): the cofactors of the symmetric matrix
  const i128 c00 = s2 * s0 - s1 * s1, c01 = s2 * s1 - s3 * s0, c02 = s3 * s1 - s2 * s2, c11 = s4 * s0 - s2 * s2, c12 = s3 * s2 - s4 * s1, c22 = s4 * s2 - s3 * s3;
  const i128 det = s4 * c00 + s3 * c01 + s2 * c02;
  if (det == 0) return false;
  out[0] = quotient_rn(c00 * t2 + c01 * t1 + c02 * t0, det);
  out[1] = quotient_rn(c01 * t2 + c11 * t1 + c12 * t0, det);
  out[2] = quotient_rn(c02 * t2 + c12 * t1 + c22 * t0, det);
  return true;
}

Lanes::Lanes(int gpu, int capacity) : gpu_(gpu), capacity_(capacity) {
  if (capacity < 1 || capacity > 4096) throw std::invalid_argument("vp_lanes_create: capacity " + std::to_string(capacity) + " (1 .. 4096)");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  try {
    VP_HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    for (hipEvent_t* ev : {&ev_src_, &ev_read_, &stage_ev_[0], &stage_ev_[1]}) VP_HIP_CHECK(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    VP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_records_), (size_t)capacity * sizeof(LaneFilterRecord)));
    VP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_points_), (size_t)capacity * 4 * kLaneRunPoints * sizeof(uint16_t)));
    VP_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&h_records_), (size_t)capacity * sizeof(LaneFilterRecord), hipHostMallocDefault));
  } catch (...) {
    release();
    throw;
  }
}

Lanes::~Lanes() { release(); }

void Lanes::release() {
  (void)hipSetDevice(gpu_);
  if (stream_) (void)hipStreamSynchronize(stream_);
  for (hipEvent_t* ev : {&ev_src_, &ev_read_, &stage_ev_[0], &stage_ev_[1]}) {
    if (*ev) (void)hipEventDestroy(*ev);
    *ev = nullptr;
  }
  if (d_records_) (void)hipFree(d_records_);
  if (d_points_) (void)hipFree(d_points_);
  if (h_records_) (void)hipHostFree(h_records_);
  h_records_ = nullptr;
  if (d_stage_) (void)hipFree(d_stage_);
  if (h_stage_) (void)hipHostFree(h_stage_);
  d_records_ = nullptr;
  d_points_ = nullptr;
  d_stage_ = h_stage_ = nullptr;
  if (stream_) (void)hipStreamDestroy(stream_);
  stream_ = nullptr;
}

void Lanes::reset() {
  if (count_) throw std::runtime_error("vp_lanes_reset: " + std::to_string(count_) + " records are pending (vp_lanes_fetch first: the smoothing is applied as they are fetched)");
  prev_[0].valid = prev_[1].valid = false;
}

LaneFilterRecord* Lanes::next_record(const char* who) {
  if (count_ >= capacity_) throw std::runtime_error(std::string(who) + ": " + std::to_string(capacity_) + " records are pending already (vp_lanes_fetch)");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  return d_records_ + (head_ + count_) % capacity_;
}

void Lanes::launch(const float* d_logits, float threshold) {
  const int slot = (head_ + count_) % capacity_;
  LaneFilterParams q{};
  q.logits = d_logits;
  q.threshold = threshold;
  q.rec = d_records_ + slot;
  q.points = d_points_ + (size_t)slot * 4 * kLaneRunPoints;
  VP_HIP_CHECK(launch_lane_filter(q, stream_));
}

void Lanes::add(Engine& e, float threshold) {
  const std::string me("vp_lanes_add");
  if (e.gpu_ != gpu_) throw std::invalid_argument(me + ": the engine lives on GPU " + std::to_string(e.gpu_) + ", the lane filter on GPU " + std::to_string(gpu_));
  if (e.kind_ != 3) throw std::invalid_argument(me + ": VP_EGOLANES engines only (the three lane planes of its logits)");
  if (e.frames_ > 1) throw std::invalid_argument(me + ": a batched encoder has no outputs of its own (filter its per-camera heads)");
  if (!e.have_outputs_) throw std::runtime_error("Inference has not been run yet");
  if (!e.d_logits_ || e.out_c_ != 3 || e.out_h_ != kLaneH || e.out_w_ != kLaneW) throw std::invalid_argument(me + ": the engine has no logits of 3 x 80 x 160");
  next_record("vp_lanes_add");
  VP_HIP_CHECK(hipEventRecord(ev_src_, e.stream_));
  VP_HIP_CHECK(hipStreamWaitEvent(stream_, ev_src_, 0));
  launch(e.d_logits_, threshold);
  VP_HIP_CHECK(hipEventRecord(ev_read_, stream_));
  VP_HIP_CHECK(hipStreamWaitEvent(e.stream_, ev_read_, 0));
  ++count_;
}

// Metric::stage_host's scheme: the copy into a pinned slot happens before the call returns, the H2D and the kernel follow on the stream
void Lanes::add_logits(const float* host, float threshold) {
  if (!host) throw std::invalid_argument("vp_lanes_add_logits: null logits");
  next_record("vp_lanes_add_logits");
  const size_t bytes = 3 * sizeof(float) * kLaneH * kLaneW;
  if (!d_stage_) VP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_stage_), bytes));
  if (!h_stage_) VP_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&h_stage_), 2 * bytes, hipHostMallocDefault));
  stage_slot_ ^= 1;
  float* slot = h_stage_ + (size_t)stage_slot_ * 3 * kLaneH * kLaneW;
  VP_HIP_CHECK(hipEventSynchronize(stage_ev_[stage_slot_]));   // the H2D that last read this slot, two calls ago
  std::memcpy(slot, host, bytes);
  VP_HIP_CHECK(hipMemcpyAsync(d_stage_, slot, bytes, hipMemcpyHostToDevice, stream_));
  VP_HIP_CHECK(hipEventRecord(stage_ev_[stage_slot_], stream_));
  launch(d_stage_, threshold);
  ++count_;
}

void Lanes::fetch(LaneFilterRecord* recs, LanesFit* fits, int count) {
  if (count < 0 || count > count_ || (count > 0 && (!recs || !fits))) throw std::invalid_argument("vp_lanes_fetch: more records than are pending, or a null buffer");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  const int first = std::min(count, capacity_ - head_);   // the ring wraps at most once
  if (first > 0) VP_HIP_CHECK(hipMemcpyAsync(h_records_, d_records_ + head_, (size_t)first * sizeof(LaneFilterRecord), hipMemcpyDeviceToHost, stream_));
  if (count > first) VP_HIP_CHECK(hipMemcpyAsync(h_records_ + first, d_records_, (size_t)(count - first) * sizeof(LaneFilterRecord), hipMemcpyDeviceToHost, stream_));
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
  if (count) std::memcpy(recs, h_records_, (size_t)count * sizeof(LaneFilterRecord));
  head_ = (head_ + count) % capacity_;
  count_ -= count;
  for (int i = 0; i < count; ++i) {
    for (int l = 0; l < 2; ++l) {
      const LaneFilterLane& r = recs[i].lane[l];
      LanesFit& f = fits[2 * i + l];
      f = LanesFit{};
      if (r.start_x < 0) {   // no start point: the lane is lost and so is its history
        prev_[l].valid = false;
        continue;
      }
      const int n = r.n_points[0] + r.n_points[1];
      if (n < 4) continue;   // a start point but no fit: the previous fit stays as it is
      const int order = n < 30 ? 1 : 2;
      double abc[3];
      if (!lanes_fit(r.S, r.T, order, abc)) {
        f.flags |= kLanesSingular;
        continue;
      }
      f.order = order;
      f.raw[0] = 0.0, f.raw[1] = abc[0], f.raw[2] = abc[1], f.raw[3] = abc[2], f.raw[4] = (double)r.min_y, f.raw[5] = (double)r.max_y;
      for (int k = 0; k < 6; ++k) f.coeffs[k] = f.raw[k];
      if (prev_[l].valid) {
#pragma clang fp contract(off)
        const double s = (double)smoothing_, t = (double)(1.0f - smoothing_);   // the reference's float factors, products and sum in double
        for (int k = 0; k < 6; ++k) {
          const double a = s * f.raw[k], b = t * prev_[l].c[k];
          f.coeffs[k] = a + b;
        }
        f.flags |= kLanesSmoothed;
      }
      prev_[l].valid = true;
      for (int k = 0; k < 6; ++k) prev_[l].c[k] = f.coeffs[k];
      f.coeffs_valid = 1;
    }
  }
}

int Lanes::fetch_points(int index, int lane, uint8_t* xy, int max_points) {
  if (count_ < 1) throw std::runtime_error("vp_lanes_fetch_points: no record is pending (the points of a record last until vp_lanes_fetch returns it)");
  if (index < 0 || index >= count_ || (lane != 0 && lane != 1) || max_points < 0 || (max_points > 0 && !xy))
    throw std::invalid_argument("vp_lanes_fetch_points: record_index outside the pending records, lane not 0 or 1, or a null buffer");
  VP_HIP_CHECK(hipSetDevice(gpu_));
  const int slot = (head_ + index) % capacity_;
  int np[2];
  VP_HIP_CHECK(hipMemcpyAsync(np, reinterpret_cast<const uint8_t*>(d_records_ + slot) + offsetof(LaneFilterRecord, lane) + (size_t)lane * sizeof(LaneFilterLane) + offsetof(LaneFilterLane, n_points),
                              sizeof(np), hipMemcpyDeviceToHost, stream_));
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
  if (np[0] < 0 || np[0] > kLaneRunPoints || np[1] < 0 || np[1] > kLaneRunPoints) throw std::runtime_error("vp_lanes_fetch_points: a point count outside 0 .. 960 in the record");
  const int total = np[0] + np[1], n = std::min(total, max_points), up = std::min(np[0], n);
  const uint16_t* base = d_points_ + ((size_t)slot * 4 + (size_t)lane * 2) * kLaneRunPoints;   // x | y << 8, little endian: the byte pairs (x, y)
  if (up > 0) VP_HIP_CHECK(hipMemcpyAsync(xy, base, (size_t)up * 2, hipMemcpyDeviceToHost, stream_));
  if (n > up) VP_HIP_CHECK(hipMemcpyAsync(xy + (size_t)up * 2, base + kLaneRunPoints, (size_t)(n - up) * 2, hipMemcpyDeviceToHost, stream_));
  VP_HIP_CHECK(hipStreamSynchronize(stream_));
  return total;
}

}  // namespace vp

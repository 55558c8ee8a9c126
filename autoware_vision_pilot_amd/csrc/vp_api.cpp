// C ABI of libvp_hip.so (declarations + reference citations: include/vp_hip.h).  No exception crosses it.
#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <fstream>

#include "vp_handle.hpp"
#include "engine_internal.hpp"

namespace {

void set_err(char* err, size_t n, const std::string& msg) {
  if (err && n) {
    std::snprintf(err, n, "%s", msg.c_str());
  }
}

template <class F>
int guarded(vp_engine* e, F&& f) {
  if (!e || !e->impl) return VP_ERR_ARG;
  try {
    f(*e->impl);
    return VP_OK;
  } catch (const std::invalid_argument& ex) {
    e->err = ex.what();
    return VP_ERR_ARG;
  } catch (const vp::RangeError& ex) {
    e->err = ex.what();
    return VP_ERR_RANGE;
  } catch (const std::exception& ex) {
    e->err = ex.what();
    return std::strncmp(ex.what(), "HIP error", 9) == 0 ? VP_ERR_HIP : VP_ERR_STATE;
  }
}

int create_impl(vp_engine** out, int kind, const void* blob, size_t bytes, int precision, int gpu_id, char* err, size_t err_len,
                vp::Engine* base = nullptr, int frames = 1, int frame_index = 0) {
  if (!out) return VP_ERR_ARG;
  *out = nullptr;
  try {
    vp::WeightBlob wb;
    try {
      wb.parse(blob, bytes);
    } catch (const std::exception& ex) {
      set_err(err, err_len, ex.what());
      return VP_ERR_WEIGHTS;
    }
    auto h = std::make_unique<vp_engine>();
    try {
      h->impl = std::make_unique<vp::Engine>(kind, &wb, precision, gpu_id, base, frames, frame_index);
    } catch (const std::invalid_argument& ex) {
      set_err(err, err_len, ex.what());
      return VP_ERR_ARG;
    } catch (const vp::RangeError& ex) {   // a folded weight beyond the fp16 range
      set_err(err, err_len, ex.what());
      return VP_ERR_RANGE;
    } catch (const std::exception& ex) {
      set_err(err, err_len, ex.what());
      return std::strstr(ex.what(), "weight") ? VP_ERR_WEIGHTS : VP_ERR_HIP;
    }
    *out = h.release();
    return VP_OK;
  } catch (...) {
    set_err(err, err_len, "unknown failure");
    return VP_ERR_STATE;
  }
}

// Weight file -> VPW1 bytes.  `*.onnx` (the reference's `model_path`, ROS2/models/config/autoseg.yaml:3) goes through
// the native ONNX reader; anything else is read as a VPW1 blob.
int read_weights(const char* path, std::vector<char>& buf, char* err, size_t err_len) {
  const std::string p(path);
  auto ends_with = [&](const char* suf) {
    const size_t n = std::strlen(suf);
    if (p.size() < n) return false;
    for (size_t i = 0; i < n; ++i)
      if (std::tolower((unsigned char)p[p.size() - n + i]) != suf[i]) return false;
    return true;
  };
  if (ends_with(".onnx")) {
    try {
      buf = vp::onnx_to_blob(p);
      return VP_OK;
    } catch (const std::exception& ex) {
      set_err(err, err_len, ex.what());
      return VP_ERR_WEIGHTS;
    }
  }
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) {
    set_err(err, err_len, std::string("cannot open weight file: ") + path);
    return VP_ERR_WEIGHTS;
  }
  const std::streamsize n = f.tellg();
  f.seekg(0);
  buf.resize((size_t)n);
  if (n && !f.read(buf.data(), n)) {
    set_err(err, err_len, "short read on weight file");
    return VP_ERR_WEIGHTS;
  }
  return VP_OK;
}

}  // namespace

extern "C" {

// Stateless twin of MasksVisualizationKernels::createMaskFromTensor{CUDA,HIP} / createEgoLanesMaskFromTensorCUDA
// (common/include/masks_visualization_kernels.hpp:14-45, masks_viz.hip.cpp:41-97): HOST logits up, decode kernel, mask down.
// Same shape of work as the reference helper (allocate, copy, launch, copy, free); the engine-resident path (vp_mask_u8)
// never re-uploads the logits.
int vp_decode_logits_host(int gpu_id, const float* logits_nchw, int channels, int h, int w, int decode_mode, uint8_t* mask_out) {
  if (!logits_nchw || !mask_out || channels < 1 || h < 1 || w < 1 || decode_mode < 0 || decode_mode > 2) return VP_ERR_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || gpu_id < 0 || gpu_id >= ndev) return VP_ERR_HIP;
  if (hipSetDevice(gpu_id) != hipSuccess) return VP_ERR_HIP;
  const size_t hw = (size_t)h * w, in_bytes = hw * channels * sizeof(float);
  float* d_in = nullptr;
  uint8_t* d_out = nullptr;
  hipStream_t st = nullptr;
  int rc = VP_ERR_HIP;
  if (hipMalloc(reinterpret_cast<void**>(&d_in), in_bytes) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&d_out), hw) == hipSuccess &&
      hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess &&
      hipMemcpyAsync(d_in, logits_nchw, in_bytes, hipMemcpyHostToDevice, st) == hipSuccess &&
      vp::launch_decode_mask(d_in, channels, (int)hw, decode_mode, d_out, st) == hipSuccess &&
      hipMemcpyAsync(mask_out, d_out, hw, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess)
    rc = VP_OK;
  if (st) hipStreamDestroy(st);
  if (d_in) hipFree(d_in);
  if (d_out) hipFree(d_out);
  return rc;
}


int vp_create_from_memory(vp_engine** out, int model_kind, const void* blob, size_t blob_bytes, int precision, int gpu_id, char* err,
                          size_t err_len) {
  if (!blob) {
    set_err(err, err_len, "null weight blob");
    return VP_ERR_ARG;
  }
  return create_impl(out, model_kind, blob, blob_bytes, precision, gpu_id, err, err_len);
}

int vp_create(vp_engine** out, int model_kind, const char* weights_path, int precision, int gpu_id, char* err, size_t err_len) {
  if (!weights_path || !*weights_path) {
    set_err(err, err_len, "No path to weight file provided");  // scene_seg_infer.py:33
    return VP_ERR_ARG;
  }
  std::vector<char> buf;
  if (const int rc = read_weights(weights_path, buf, err, err_len)) return rc;
  return create_impl(out, model_kind, buf.data(), buf.size(), precision, gpu_id, err, err_len);
}

int vp_create_shared_from_memory(vp_engine** out, vp_engine* base, int model_kind, const void* blob, size_t blob_bytes, int precision,
                                 int gpu_id, char* err, size_t err_len) {
  if (!blob || !base || !base->impl) {
    set_err(err, err_len, !blob ? "null weight blob" : "null base engine");
    return VP_ERR_ARG;
  }
  return create_impl(out, model_kind, blob, blob_bytes, precision, gpu_id, err, err_len, base->impl.get());
}

int vp_create_shared(vp_engine** out, vp_engine* base, int model_kind, const char* weights_path, int precision, int gpu_id, char* err,
                     size_t err_len) {
  if (!weights_path || !*weights_path) {
    set_err(err, err_len, "No path to weight file provided");
    return VP_ERR_ARG;
  }
  std::vector<char> buf;
  if (const int rc = read_weights(weights_path, buf, err, err_len)) return rc;
  return vp_create_shared_from_memory(out, base, model_kind, buf.data(), buf.size(), precision, gpu_id, err, err_len);
}

int vp_create_batched_from_memory(vp_engine** out, int model_kind, const void* blob, size_t blob_bytes, int precision, int gpu_id, int frames,
                                  char* err, size_t err_len) {
  if (!blob) {
    set_err(err, err_len, "null weight blob");
    return VP_ERR_ARG;
  }
  return create_impl(out, model_kind, blob, blob_bytes, precision, gpu_id, err, err_len, nullptr, frames, 0);
}

int vp_create_batched(vp_engine** out, int model_kind, const char* weights_path, int precision, int gpu_id, int frames, char* err,
                      size_t err_len) {
  if (!weights_path || !*weights_path) {
    set_err(err, err_len, "No path to weight file provided");
    return VP_ERR_ARG;
  }
  std::vector<char> buf;
  if (const int rc = read_weights(weights_path, buf, err, err_len)) return rc;
  return create_impl(out, model_kind, buf.data(), buf.size(), precision, gpu_id, err, err_len, nullptr, frames, 0);
}

int vp_create_shared_frame_from_memory(vp_engine** out, vp_engine* base, int frame_index, int model_kind, const void* blob, size_t blob_bytes,
                                       int precision, int gpu_id, char* err, size_t err_len) {
  if (!blob || !base || !base->impl) {
    set_err(err, err_len, !blob ? "null weight blob" : "null base engine");
    return VP_ERR_ARG;
  }
  return create_impl(out, model_kind, blob, blob_bytes, precision, gpu_id, err, err_len, base->impl.get(), 1, frame_index);
}

int vp_create_shared_frame(vp_engine** out, vp_engine* base, int frame_index, int model_kind, const char* weights_path, int precision,
                           int gpu_id, char* err, size_t err_len) {
  if (!weights_path || !*weights_path) {
    set_err(err, err_len, "No path to weight file provided");
    return VP_ERR_ARG;
  }
  std::vector<char> buf;
  if (const int rc = read_weights(weights_path, buf, err, err_len)) return rc;
  return vp_create_shared_frame_from_memory(out, base, frame_index, model_kind, buf.data(), buf.size(), precision, gpu_id, err, err_len);
}

int vp_frames(const vp_engine* e) { return (e && e->impl) ? e->impl->frames() : -1; }

int vp_upload_frame_n(vp_engine* e, int index, const uint8_t* frame, int h, int w, int stride_bytes) {
  return guarded(e, [&](vp::Engine& g) { g.upload_frame(frame, h, w, stride_bytes, index); });
}

int vp_convert_onnx(const char* onnx_path, const char* vpw_path, char* err, size_t err_len) {
  if (!onnx_path || !*onnx_path || !vpw_path || !*vpw_path) {
    set_err(err, err_len, "No path to weight file provided");
    return VP_ERR_ARG;
  }
  try {
    const std::vector<char> blob = vp::onnx_to_blob(onnx_path);
    std::ofstream o(vpw_path, std::ios::binary | std::ios::trunc);
    if (!o || !o.write(blob.data(), (std::streamsize)blob.size())) {
      set_err(err, err_len, std::string("cannot write ") + vpw_path);
      return VP_ERR_WEIGHTS;
    }
    return VP_OK;
  } catch (const std::exception& ex) {
    set_err(err, err_len, ex.what());
    return VP_ERR_WEIGHTS;
  }
}

int vp_shared_level(const vp_engine* e) { return (e && e->impl) ? e->impl->shared_level() : -1; }

int vp_infer_shared(vp_engine* e) {
  return guarded(e, [&](vp::Engine& g) {
    if (g.shared_level() == 0) throw std::invalid_argument("vp_infer_shared: not a shared-prefix engine");
    g.enqueue();
    g.fetch_outputs();
  });
}

void vp_destroy(vp_engine* e) { delete e; }

const char* vp_last_error(const vp_engine* e) { return e ? e->err.c_str() : "null engine"; }

int vp_set_input_format(vp_engine* e, int pixel_format, int plane_order) {
  return guarded(e, [&](vp::Engine& g) { g.set_input_format(pixel_format, plane_order); });
}
int vp_set_decode_mode(vp_engine* e, int mode) {
  return guarded(e, [&](vp::Engine& g) { g.set_decode_mode(mode); });
}
int vp_set_resize_mode(vp_engine* e, int mode) {
  return guarded(e, [&](vp::Engine& g) { g.set_resize_mode(mode); });
}
// host only: the tap tables the VP_RESIZE_PIL_* modes use for one axis (tests pin them against Pillow's through the oracle)
int vp_resample_coeffs(int in_size, int out_size, int resize_mode, int* bounds, int* coeffs, int coeffs_cap) {
  if (in_size < 1 || out_size < 1 || (resize_mode != 1 && resize_mode != 2) || !bounds || !coeffs) return VP_ERR_ARG;
  std::vector<int> b, k;
  const int ksize = vp::pil_coeffs(in_size, out_size, resize_mode, &b, &k);
  if ((long long)ksize * out_size > coeffs_cap) return VP_ERR_ARG;
  std::copy(b.begin(), b.end(), bounds);
  std::copy(k.begin(), k.end(), coeffs);
  return ksize;
}
int vp_set_norm_form(vp_engine* e, int form) {
  return guarded(e, [&](vp::Engine& g) { g.set_norm_form(form); });
}
int vp_get_norm_form(const vp_engine* e) { return (e && e->impl) ? e->impl->norm_form() : VP_ERR_ARG; }
int vp_set_lane_ring(vp_engine* e, int enable) {
  return guarded(e, [&](vp::Engine& g) { g.set_lane_ring(enable != 0); });
}
int vp_lane_ring_device(const vp_engine* e, void** dev_f32, int* frames_valid) {
  if (!e || !e->impl || !e->impl->lane_ring()) return VP_ERR_STATE;
  if (dev_f32) *dev_f32 = e->impl->dev_lane_ring();
  if (frames_valid) *frames_valid = e->impl->lane_ring_frames();
  return VP_OK;
}
int vp_lane_ring_fetch(vp_engine* e, float* dst_host, int* frames_valid) {
  const int rc = guarded(e, [&](vp::Engine& g) { g.fetch_lane_ring(dst_host); });
  if (rc == VP_OK && frames_valid) *frames_valid = e->impl->lane_ring_frames();
  return rc;
}
int vp_get_resize_mode(const vp_engine* e) { return (e && e->impl) ? e->impl->resize_mode() : VP_ERR_ARG; }
int vp_device_count(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}
int vp_get_decode_mode(const vp_engine* e) { return (e && e->impl) ? e->impl->decode_mode() : VP_ERR_ARG; }
int vp_gpu_id(const vp_engine* e) { return (e && e->impl) ? e->impl->gpu() : VP_ERR_ARG; }
int vp_host_logits_current(const vp_engine* e) { return (e && e->impl) ? (e->impl->host_logits_current() ? 1 : 0) : VP_ERR_ARG; }
int vp_input_hw(const vp_engine* e, int* h, int* w) {
  if (!e || !e->impl || !h || !w) return VP_ERR_ARG;
  *h = e->impl->net_h();
  *w = e->impl->net_w();
  return VP_OK;
}

int vp_infer(vp_engine* e, const uint8_t* frame, int h, int w, int stride_bytes) {
  return guarded(e, [&](vp::Engine& g) {
    g.upload_frame(frame, h, w, stride_bytes);
    g.enqueue();
    g.fetch_outputs();
  });
}
int vp_set_outputs(vp_engine* e, int outputs) {
  return guarded(e, [&](vp::Engine& g) { g.set_outputs(outputs); });
}
int vp_set_finite_check(vp_engine* e, int enable) {
  return guarded(e, [&](vp::Engine& g) { g.set_finite_check(enable != 0); });
}
int vp_set_pinned_staging(vp_engine* e, int enable) {
  return guarded(e, [&](vp::Engine& g) { g.set_pinned_staging(enable != 0); });
}
int vp_register_frames(const void* pool, size_t bytes) {
  try {
    return vp::register_frame_range(pool, bytes);
  } catch (...) {
    return VP_ERR_HIP;
  }
}
int vp_unregister_frames(const void* pool) {
  try {
    return vp::unregister_frame_range(pool);
  } catch (...) {
    return VP_ERR_HIP;
  }
}
// the same four numbers from creation on: the plan fixes them (vp_output_shape answers only after an inference, as the reference backend does)
int vp_output_dims(const vp_engine* e, int64_t shape[4]) {
  if (!e || !e->impl || !shape) return VP_ERR_ARG;
  shape[0] = 1;
  shape[1] = e->impl->out_c();
  shape[2] = e->impl->out_h();
  shape[3] = e->impl->out_w();
  return VP_OK;
}
int vp_output_shape(const vp_engine* e, int64_t shape[4]) {
  if (!e || !e->impl || !shape) return VP_ERR_ARG;
  if (!e->impl->have_outputs()) {
    const_cast<vp_engine*>(e)->err = "Inference has not been run yet. Call vp_infer() first.";  // onnx_runtime_backend.cpp:86-88
    return VP_ERR_STATE;
  }
  shape[0] = 1;
  shape[1] = e->impl->out_c();
  shape[2] = e->impl->out_h();
  shape[3] = e->impl->out_w();
  return VP_OK;
}
int vp_frame_hw(const vp_engine* e, int* h, int* w) {
  if (!e || !e->impl || !h || !w) return VP_ERR_ARG;
  *h = e->impl->frame_h();
  *w = e->impl->frame_w();
  return VP_OK;
}
// One camera frame through a base engine and its shared-prefix heads: ONE H2D, every network enqueued back to back on the
// base engine's stream, the selected outputs of every engine copied D2H behind them, ONE host synchronisation.
int vp_infer_multi(vp_engine* base, vp_engine* const* shared, int n_shared, const uint8_t* frame, int h, int w, int stride_bytes) {
  if (n_shared < 0 || (n_shared > 0 && !shared)) return VP_ERR_ARG;
  for (int i = 0; i < n_shared; ++i)
    if (!shared[i] || !shared[i]->impl) return VP_ERR_ARG;
  return guarded(base, [&](vp::Engine& g) {
    for (int i = 0; i < n_shared; ++i)
      if (shared[i]->impl->shared_level() == 0 || shared[i]->impl->stream() != g.stream())
        throw std::invalid_argument("vp_infer_multi: every head must be a shared-prefix engine of this base");
    g.upload_frame(frame, h, w, stride_bytes);
    std::vector<vp::Engine*> heads;
    for (int i = 0; i < n_shared; ++i) heads.push_back(shared[i]->impl.get());
    g.enqueue_multi(heads);
    g.enqueue_fetch();
    for (int i = 0; i < n_shared; ++i) shared[i]->impl->enqueue_fetch();
    // one synchronisation, then EVERY member's verdict is collected (and thereby consumed) before anything is thrown: a bad frame is
    // reported once, and no member keeps a stale flag for the next frame
    VP_HIP_CHECK(hipStreamSynchronize(g.stream()));
    bool bad = g.poll_status();
    for (int i = 0; i < n_shared; ++i) bad = shared[i]->impl->poll_status() || bad;
    if (bad)
      throw vp::RangeError("non-finite value (inf / NaN) in a network output of this frame: an activation left the fp16 range of the matrix pipe "
                           "(|x| > 65504) or the input / weights were not finite; outputs of this frame are invalid");
  });
}
int vp_enqueue_multi(vp_engine* base, vp_engine* const* shared, int n_shared) {
  if (n_shared < 0 || (n_shared > 0 && !shared)) return VP_ERR_ARG;
  for (int i = 0; i < n_shared; ++i)
    if (!shared[i] || !shared[i]->impl) return VP_ERR_ARG;
  return guarded(base, [&](vp::Engine& g) {
    std::vector<vp::Engine*> heads;
    for (int i = 0; i < n_shared; ++i) heads.push_back(shared[i]->impl.get());
    g.enqueue_multi(heads);
  });
}
int vp_set_multi_fork(vp_engine* base, int enable) {
  return guarded(base, [&](vp::Engine& g) { g.set_multi_fork(enable != 0); });
}
int vp_infer_pair(vp_engine* e, const uint8_t* prev, const uint8_t* curr, int h, int w, int stride_bytes) {
  return guarded(e, [&](vp::Engine& g) {
    g.upload_frame(prev, h, w, stride_bytes);
    g.stash_previous_frame();   // VP_ACT_SCALE engines keep it for vp_calibrate_range; a no-op otherwise
    g.prime_previous();
    g.upload_frame(curr, h, w, stride_bytes);
    g.enqueue();
    g.fetch_outputs();
  });
}
int vp_infer_tensor(vp_engine* e, const float* nchw) {
  return guarded(e, [&](vp::Engine& g) {
    g.upload_tensor(nchw);
    g.enqueue();
    g.fetch_outputs();
  });
}
int vp_logits(const vp_engine* e, const float** data, int64_t shape[4]) {
  if (!e || !e->impl || !data || !shape) return VP_ERR_ARG;
  if (!e->impl->have_outputs()) {
    const_cast<vp_engine*>(e)->err = "Inference has not been run yet. Call vp_infer() first.";  // onnx_runtime_backend.cpp:86-88
    return VP_ERR_STATE;
  }
  try {
    *data = e->impl->host_logits();
  } catch (const std::exception& ex) {
    const_cast<vp_engine*>(e)->err = ex.what();
    return VP_ERR_HIP;
  }
  shape[0] = 1;
  shape[1] = e->impl->out_c();
  shape[2] = e->impl->out_h();
  shape[3] = e->impl->out_w();
  return VP_OK;
}
int vp_mask_u8(const vp_engine* e, const uint8_t** data, int* h, int* w) {
  if (!e || !e->impl || !data || !h || !w) return VP_ERR_ARG;
  if (!e->impl->have_outputs()) {
    const_cast<vp_engine*>(e)->err = "Inference has not been run yet. Call vp_infer() first.";
    return VP_ERR_STATE;
  }
  try {
    *data = e->impl->host_mask();
  } catch (const std::exception& ex) {
    const_cast<vp_engine*>(e)->err = ex.what();
    return VP_ERR_HIP;
  }
  *h = e->impl->out_h();
  *w = e->impl->out_w();
  return VP_OK;
}
int vp_mask_resized_u8(vp_engine* e, uint8_t* dst, int h, int w) {
  return guarded(e, [&](vp::Engine& g) { g.mask_resized(dst, h, w); });
}
int vp_depth_resized_f32(vp_engine* e, float* dst, int h, int w) {
  return guarded(e, [&](vp::Engine& g) { g.depth_resized(dst, h, w); });
}
int vp_visualize_depth_bgr8(vp_engine* e, uint8_t* dst, int h, int w) {
  return guarded(e, [&](vp::Engine& g) { g.visualize_depth(dst, h, w); });
}
int vp_visualize_mask_bgr8(vp_engine* e, int viz_type, uint8_t* dst, int h, int w) {
  return guarded(e, [&](vp::Engine& g) { g.visualize_mask(viz_type, dst, h, w); });
}
int vp_input_tensor(vp_engine* e, float* dst) {
  return guarded(e, [&](vp::Engine& g) { g.read_input_tensor(dst); });
}

int vp_upload_frame(vp_engine* e, const uint8_t* frame, int h, int w, int stride_bytes) {
  return guarded(e, [&](vp::Engine& g) { g.upload_frame(frame, h, w, stride_bytes); });
}
int vp_enqueue(vp_engine* e) {
  return guarded(e, [&](vp::Engine& g) { g.enqueue(); });
}

// ---- vp_frame: a device-resident camera frame (include/vp_hip.h; handle: vp_handle.hpp; kernel: kernels_misc.hip frame_to_bgr8_kernel)
}  // extern "C"

vp_frame::~vp_frame() {
  (void)hipSetDevice(gpu);
  if (stream) (void)hipStreamSynchronize(stream);
  for (Consumer& c : consumers) {
    (void)hipEventSynchronize(c.done);   // a consumer's copy may still read the image
    (void)hipEventDestroy(c.done);
  }
  for (hipEvent_t ev : {stage_ev[0], stage_ev[1], ready, producer})
    if (ev) (void)hipEventDestroy(ev);
  if (d_bgr) (void)hipFree(d_bgr);
  if (d_src) (void)hipFree(d_src);
  for (void* p : {(void*)d_raw, (void*)d_mid, (void*)d_map[0], (void*)d_map[1], (void*)d_lut})
    if (p) (void)hipFree(p);
  if (h_stage) (void)hipHostFree(h_stage);
  if (stream) (void)hipStreamDestroy(stream);
}

vp::FrameView vp_frame::view() const {
  vp::FrameView v;
  v.bgr = uploaded ? d_bgr : nullptr;
  v.h = h;
  v.w = w;
  v.pitch = pitch;
  v.gpu = gpu;
  v.ready = ready;
  return v;
}

void vp_frame::note_consumer(hipStream_t s) {
  std::lock_guard<std::mutex> lk(mu);
  Consumer* c = nullptr;
  for (Consumer& k : consumers)
    if (k.stream == s) c = &k;
  if (!c) {
    hipEvent_t ev = nullptr;
    VP_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    consumers.push_back({s, ev, false});
    c = &consumers.back();
  }
  VP_HIP_CHECK(hipEventRecord(c->done, s));
  c->pending = true;
}

void vp_frame::wait_for_consumers() {
  std::lock_guard<std::mutex> lk(mu);
  for (Consumer& c : consumers)
    if (c.pending) {
      VP_HIP_CHECK(hipStreamWaitEvent(stream, c.done, 0));
      c.pending = false;
    }
}

namespace {

template <class F>
int frame_guarded(vp_frame* f, F&& fn) {
  if (!f) return VP_ERR_ARG;
  try {
    VP_HIP_CHECK(hipSetDevice(f->gpu));
    fn();
    return VP_OK;
  } catch (const std::invalid_argument& ex) {
    f->err = ex.what();
    return VP_ERR_ARG;
  } catch (const std::exception& ex) {
    f->err = ex.what();
    return std::strncmp(ex.what(), "HIP error", 9) == 0 ? VP_ERR_HIP : VP_ERR_STATE;
  }
}

struct FramePlanes {
  int n = 1;
  size_t row_bytes[3] = {0, 0, 0};
  int rows[3] = {0, 0, 0};
};

const char* const kFormatNames[vp::kFrameFormats] = {"BGR8", "RGB8", "BGRA8", "RGBA8", "GRAY8", "NV12", "YUY2", "UYVY", "I420", "YV12", "NV21"};

int format_planes(int format) { return vp::frame_format_planar(format) ? 3 : (vp::frame_format_420(format) ? 2 : 1); }

// the planes an h x w image has in `format` (vp_frame_upload*, vp_canvas_layout* / vp_canvas_fetch), and the refusals of the geometry
// min_side: 2 for a frame or a canvas; 1 for the resized picture of vp_canvas_fetch_resized
FramePlanes frame_layout(const std::string& me, int format, int h, int w, int min_side = 2) {
  static const int px_bytes[vp::kFrameFormats] = {3, 3, 4, 4, 1, 1, 2, 2, 1, 1, 1};
  const int fi = vp::frame_format_index(format);
  if (fi < 0) throw std::invalid_argument(me + ": unknown format " + std::to_string(format));
  const std::string fmt = kFormatNames[fi];
  if (h < min_side || w < min_side || h > 16384 || w > 16384)
    throw std::invalid_argument(me + ": frame size " + std::to_string(w) + " x " + std::to_string(h) + " (" + std::to_string(min_side) + " .. 16384 each way)");
  if (format >= VP_FRAME_NV12 && (w & 1)) throw std::invalid_argument(me + ": " + fmt + " needs an even width (one chroma pair per two pixels), got " + std::to_string(w));
  if (vp::frame_format_420(format) && (h & 1)) throw std::invalid_argument(me + ": " + fmt + " needs an even height (one chroma pair per 2x2 block), got " + std::to_string(h));
  FramePlanes fp;
  fp.n = format_planes(format);
  fp.row_bytes[0] = (size_t)px_bytes[fi] * w;
  fp.rows[0] = h;
  for (int i = 1; i < fp.n; ++i) {
    fp.row_bytes[i] = fp.n == 2 ? (size_t)w : (size_t)w / 2;   // w / 2 interleaved pairs, or w / 2 samples of one plane
    fp.rows[i] = h / 2;
  }
  return fp;
}

// the refusals of vp_frame_upload* / vp_canvas_fetch, and the planes the format has
FramePlanes check_frame_planes(const char* who, int format, const void* const* planes, const int* strides, int n_planes, int h, int w, int min_side = 2) {
  const std::string me(who);
  const int fi = vp::frame_format_index(format);
  if (fi < 0) throw std::invalid_argument(me + ": unknown format " + std::to_string(format));
  const int n = format_planes(format);
  if (n_planes != n) throw std::invalid_argument(me + ": " + kFormatNames[fi] + " has " + std::to_string(n) + " plane(s), got n_planes = " + std::to_string(n_planes));
  if (!planes || !strides) throw std::invalid_argument(me + ": null planes / strides");
  const FramePlanes fp = frame_layout(me, format, h, w, min_side);
  for (int i = 0; i < fp.n; ++i) {
    if (!planes[i]) throw std::invalid_argument(me + ": plane " + std::to_string(i) + " is null");
    if (strides[i] < 0 || (size_t)strides[i] < fp.row_bytes[i])
      throw std::invalid_argument(me + ": stride " + std::to_string(strides[i]) + " of plane " + std::to_string(i) + " is below the row's " + std::to_string(fp.row_bytes[i]) + " bytes");
  }
  return fp;
}

// ---- the upload-only formats (GRAY16, P010, raw Bayer): layouts and refusals of their own, so vp_canvas_* keeps answering "unknown format" for them
bool upload_only_format(int format) { return vp::frame_format_deep(format) || vp::frame_format_bayer(format); }
std::string upload_only_name(int format) {
  static const char* const order[4] = {"RGGB", "GRBG", "GBRG", "BGGR"};
  if (format == VP_FRAME_GRAY16) return "GRAY16";
  if (format == VP_FRAME_P010) return "P010";
  return std::string("BAYER_") + order[(format - VP_FRAME_BAYER_RGGB8) & 3] + (vp::frame_format_bayer16(format) ? "16" : "8");
}
// B of the definition (include/vp_hip.h) for a Bayer upload under the frame's raw setting, and the refusals that need B
int raw_significant_bits(const std::string& me, const vp_frame* f, int format) {
  const vp_raw& r = f->raw;
  const bool wide = vp::frame_format_bayer16(format);
  const std::string fmt = upload_only_name(format);
  if (r.bits == 8 && wide) throw std::invalid_argument(me + ": the raw setting's bits = 8 does not fit " + fmt + " (16-bit words: 10, 12, 14, 16 or 0)");
  if (r.bits > 8 && !wide) throw std::invalid_argument(me + ": the raw setting's bits = " + std::to_string(r.bits) + " does not fit " + fmt + " (bytes: 8 or 0)");
  const int B = r.bits ? r.bits : (wide ? 16 : 8), M = (1 << B) - 1;
  if (r.black > M) throw std::invalid_argument(me + ": the raw setting's black = " + std::to_string(r.black) + " is above the " + std::to_string(B) + "-bit maximum " + std::to_string(M));
  if (r.lut_len && r.lut_len != 1 << (B < 12 ? B : 12))
    throw std::invalid_argument(me + ": the raw setting's LUT has " + std::to_string(r.lut_len) + " entries, " + std::to_string(B) + "-bit samples need " + std::to_string(1 << (B < 12 ? B : 12)));
  return B;
}
FramePlanes check_upload_only_planes(const std::string& me, const vp_frame* f, int format, const void* const* planes, const int* strides, int n_planes, int h, int w) {
  const std::string fmt = upload_only_name(format);
  const bool p010 = format == VP_FRAME_P010, bayer = vp::frame_format_bayer(format), wide = !bayer || vp::frame_format_bayer16(format);
  const int n = p010 ? 2 : 1;
  if (n_planes != n) throw std::invalid_argument(me + ": " + fmt + " has " + std::to_string(n) + " plane(s), got n_planes = " + std::to_string(n_planes));
  if (!planes || !strides) throw std::invalid_argument(me + ": null planes / strides");
  if (h < 2 || w < 2 || h > 16384 || w > 16384) throw std::invalid_argument(me + ": frame size " + std::to_string(w) + " x " + std::to_string(h) + " (2 .. 16384 each way)");
  const char* why = p010 ? "one chroma pair per 2x2 block" : "whole 2x2 CFA cells";
  if (format != VP_FRAME_GRAY16 && (w & 1)) throw std::invalid_argument(me + ": " + fmt + " needs an even width (" + why + "), got " + std::to_string(w));
  if (format != VP_FRAME_GRAY16 && (h & 1)) throw std::invalid_argument(me + ": " + fmt + " needs an even height (" + why + "), got " + std::to_string(h));
  FramePlanes fp;
  fp.n = n;
  fp.row_bytes[0] = (size_t)(wide ? 2 : 1) * w;
  fp.rows[0] = h;
  if (p010) {
    fp.row_bytes[1] = 2 * (size_t)w;   // w / 2 pairs of U V words
    fp.rows[1] = h / 2;
  }
  for (int i = 0; i < fp.n; ++i) {
    if (!planes[i]) throw std::invalid_argument(me + ": plane " + std::to_string(i) + " is null");
    if (strides[i] < 0 || (size_t)strides[i] < fp.row_bytes[i])
      throw std::invalid_argument(me + ": stride " + std::to_string(strides[i]) + " of plane " + std::to_string(i) + " is below the row's " + std::to_string(fp.row_bytes[i]) + " bytes");
    if (wide && (strides[i] & 1)) throw std::invalid_argument(me + ": stride " + std::to_string(strides[i]) + " of plane " + std::to_string(i) + " is odd: " + fmt + " holds 16-bit words");
    if (wide && (reinterpret_cast<uintptr_t>(planes[i]) & 1)) throw std::invalid_argument(me + ": plane " + std::to_string(i) + " lies at an odd address: " + fmt + " holds 16-bit words");
  }
  if (bayer) (void)raw_significant_bits(me, f, format);
  return fp;
}
// every refusal of vp_frame_upload* ahead of the first change to the frame
FramePlanes check_upload(const char* who, const vp_frame* f, int format, const void* const* planes, const int* strides, int n_planes, int h, int w) {
  if (upload_only_format(format)) return check_upload_only_planes(who, f, format, planes, strides, n_planes, h, w);
  return check_frame_planes(who, format, planes, strides, n_planes, h, w);
}

void check_color(const std::string& me, int matrix, int range) {
  if (matrix != VP_COLOR_BT601 && matrix != VP_COLOR_BT709) throw std::invalid_argument(me + ": unknown colour matrix " + std::to_string(matrix) + " (VP_COLOR_BT601, VP_COLOR_BT709)");
  if (range != VP_COLOR_RANGE_LIMITED && range != VP_COLOR_RANGE_FULL) throw std::invalid_argument(me + ": unknown colour range " + std::to_string(range) + " (VP_COLOR_RANGE_LIMITED, VP_COLOR_RANGE_FULL)");
}

template <class T>
void grow(T*& p, size_t& cap, size_t need, bool pinned) {
  if (need <= cap) return;
  if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
  p = nullptr;
  cap = 0;
  const size_t n = (need + 255) & ~(size_t)255;
  VP_HIP_CHECK(pinned ? hipHostMalloc(reinterpret_cast<void**>(&p), n, hipHostMallocDefault) : hipMalloc(reinterpret_cast<void**>(&p), n));
  cap = n;
}

// ---- rectification maps: host code, the formulas of include/vp_hip.h in IEEE double in the order written.  `#pragma clang fp contract(off)` keeps the
// compiler from contracting a multiply and an add into one fused operation, whatever the build's flags say: the numpy restatement of the tests rounds
// after every operation, and the maps are compared bit for bit.
int coord32(double v) {   // rne (the default rounding mode), then the clamp; a NaN takes the lower clamp
  v = std::nearbyint(v);
  if (!(v >= -1048576.0)) return -1048576;
  return v > 1048575.0 ? 1048575 : (int)v;
}
void distort_point(const vp_rectify& r, double x, double y, double* u, double* v) {
#pragma clang fp contract(off)
  const double k1 = r.dist[0], k2 = r.dist[1], p1 = r.dist[2], p2 = r.dist[3], k3 = r.dist[4];
  const double r2 = x * x + y * y;
  const double kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
  const double xy2 = 2.0 * (x * y);
  const double xd = x * kr + p1 * xy2 + p2 * (r2 + 2.0 * (x * x));
  const double yd = y * kr + p1 * (r2 + 2.0 * (y * y)) + p2 * xy2;
  *u = r.K[0] * xd + r.K[2];
  *v = r.K[4] * yd + r.K[5];
}
double homography_adjugate(const double* H, double* a) {   // the nine cofactors; returns det H
#pragma clang fp contract(off)
  a[0] = H[4] * H[8] - H[5] * H[7];
  a[1] = H[2] * H[7] - H[1] * H[8];
  a[2] = H[1] * H[5] - H[2] * H[4];
  a[3] = H[5] * H[6] - H[3] * H[8];
  a[4] = H[0] * H[8] - H[2] * H[6];
  a[5] = H[2] * H[3] - H[0] * H[5];
  a[6] = H[3] * H[7] - H[4] * H[6];
  a[7] = H[1] * H[6] - H[0] * H[7];
  a[8] = H[0] * H[4] - H[1] * H[3];
  return (H[0] * a[0] + H[1] * a[3]) + H[2] * a[6];
}
bool rectify_h_is_identity(const vp_rectify& r) {
  for (int i = 0; i < 9; ++i)
    if (r.H[i] != (i % 4 == 0 ? 1.0 : 0.0)) return false;
  return true;
}
bool rectify_dist_is_zero(const vp_rectify& r) {
  for (double d : r.dist)
    if (d != 0.0) return false;
  return true;
}
void check_rectify(const std::string& me, const vp_rectify& r) {
  for (double v : r.K)
    if (!std::isfinite(v)) throw std::invalid_argument(me + ": K holds a non-finite value");
  for (double v : r.dist)
    if (!std::isfinite(v)) throw std::invalid_argument(me + ": dist holds a non-finite value");
  for (double v : r.H)
    if (!std::isfinite(v)) throw std::invalid_argument(me + ": H holds a non-finite value");
  if (r.K[0] == 0.0 || r.K[4] == 0.0) throw std::invalid_argument(me + ": fx and fy of K must not be 0");
  if (r.K[1] != 0.0 || r.K[3] != 0.0 || r.K[6] != 0.0 || r.K[7] != 0.0 || r.K[8] != 1.0)
    throw std::invalid_argument(me + ": K must be [fx 0 cx; 0 fy cy; 0 0 1] (no skew)");
  double a[9];
  const double det = homography_adjugate(r.H, a);
  if (det == 0.0 || !std::isfinite(det)) throw std::invalid_argument(me + ": det H is 0 or not finite: H has no inverse");
  if (r.out_w < 2 || r.out_h < 2 || r.out_w > 16384 || r.out_h > 16384)
    throw std::invalid_argument(me + ": output size " + std::to_string(r.out_w) + " x " + std::to_string(r.out_h) + " (2 .. 16384 each way)");
  if (r.mode != VP_RECTIFY_TWO_PASS && r.mode != VP_RECTIFY_ONE_PASS)
    throw std::invalid_argument(me + ": unknown mode " + std::to_string(r.mode) + " (VP_RECTIFY_TWO_PASS, VP_RECTIFY_ONE_PASS)");
}
void check_rectify_source(const std::string& me, int src_h, int src_w) {
  if (src_h < 2 || src_w < 2 || src_h > 16384 || src_w > 16384)
    throw std::invalid_argument(me + ": source size " + std::to_string(src_w) + " x " + std::to_string(src_h) + " (2 .. 16384 each way)");
}
// which: 0 undistort (src_h x src_w), 1 warp, 2 one-pass (both out_h x out_w); rows `pitch` entries apart
void build_rectify_map(const vp_rectify& r, int src_h, int src_w, int which, vp::RemapEntry* out, int pitch) {
#pragma clang fp contract(off)
  const double fx = r.K[0], fy = r.K[4], cx = r.K[2], cy = r.K[5];
  if (which == 0) {
    for (int i = 0; i < src_h; ++i)
      for (int j = 0; j < src_w; ++j) {
        double u, v;
        distort_point(r, ((double)j - cx) / fx, ((double)i - cy) / fy, &u, &v);
        out[(size_t)i * pitch + j] = {coord32(32.0 * u), coord32(32.0 * v)};
      }
    return;
  }
  double M[9];
  const double det = homography_adjugate(r.H, M);
  for (double& m : M) m = m / det;
  for (int yi = 0; yi < r.out_h; ++yi)
    for (int xi = 0; xi < r.out_w; ++xi) {
      const double x = (double)xi, y = (double)yi;
      const double X0 = (M[0] * x + M[1] * y) + M[2], Y0 = (M[3] * x + M[4] * y) + M[5], W = (M[6] * x + M[7] * y) + M[8];
      vp::RemapEntry& e = out[(size_t)yi * pitch + xi];
      if (which == 1) {
        const double s = W != 0.0 ? 32.0 / W : 0.0;
        const double lim = 2147483648.0;
        const double xs = X0 * s, ys = Y0 * s;
        e = {coord32(xs < -lim ? -lim : (xs > lim ? lim : xs)), coord32(ys < -lim ? -lim : (ys > lim ? lim : ys))};
      } else {
        double px = W != 0.0 ? X0 / W : 0.0, py = W != 0.0 ? Y0 / W : 0.0;
        px = px >= 0.0 ? (px > (double)(src_w - 1) ? (double)(src_w - 1) : px) : 0.0;   // a NaN takes 0
        py = py >= 0.0 ? (py > (double)(src_h - 1) ? (double)(src_h - 1) : py) : 0.0;
        double u, v;
        distort_point(r, (px - cx) / fx, (py - cy) / fy, &u, &v);
        e = {coord32(32.0 * u), coord32(32.0 * v)};
      }
    }
}

// what an upload of an h x w frame does under the frame's rectification setting: the passes that run and the picture's geometry
struct RectifyPlan {
  bool on = false;
  bool pass[2] = {false, false};   // [0]: undistort, or the one-pass map (border CONSTANT); [1]: warp (border REPLICATE)
  int out_h = 0, out_w = 0;
};
RectifyPlan rectify_plan(const vp_frame* f, int h, int w) {
  RectifyPlan p;
  p.out_h = h;
  p.out_w = w;
  if (!f->rect_on) return p;
  const vp_rectify& r = f->rect;
  p.out_h = r.out_h;
  p.out_w = r.out_w;
  if (r.mode == VP_RECTIFY_ONE_PASS) {
    p.pass[0] = true;
  } else {
    p.pass[0] = !rectify_dist_is_zero(r);
    p.pass[1] = !(rectify_h_is_identity(r) && r.out_h == h && r.out_w == w);
  }
  p.on = p.pass[0] || p.pass[1];
  return p;
}
// where the format conversion (or the BGR8 copy) of the upload in flight writes: the picture itself, or the raw-sized buffer ahead of the passes
uint8_t* conversion_target(const vp_frame* f, int h, int w) { return rectify_plan(f, h, w).on ? f->d_raw : f->d_bgr; }

// the maps of the frame's setting for an h x w source, on the device: one host computation (and one host wait) per geometry and setting
void ensure_rectify_maps(vp_frame* f, const RectifyPlan& p, int h, int w) {
  if (f->map_h == h && f->map_w == w) return;
  VP_HIP_CHECK(hipStreamSynchronize(f->stream));   // a pass queued earlier may still read the maps
  f->map_h = f->map_w = 0;
  const bool one = f->rect.mode == VP_RECTIFY_ONE_PASS;
  std::vector<vp::RemapEntry> host;
  for (int i = 0; i < 2; ++i) {
    if (!p.pass[i]) continue;
    const int mh = (i == 0 && !one) ? h : p.out_h, mw = (i == 0 && !one) ? w : p.out_w, pitch = vp::frame_remap_map_pitch(mw);
    host.assign((size_t)mh * pitch, vp::RemapEntry{0, 0});
    build_rectify_map(f->rect, h, w, i == 0 ? (one ? 2 : 0) : 1, host.data(), pitch);
    grow(f->d_map[i], f->map_cap[i], host.size() * sizeof(vp::RemapEntry), false);
    VP_HIP_CHECK(hipMemcpyAsync(f->d_map[i], host.data(), host.size() * sizeof(vp::RemapEntry), hipMemcpyHostToDevice, f->stream));
    VP_HIP_CHECK(hipStreamSynchronize(f->stream));   // `host` is pageable and about to be reused
  }
  f->map_h = h;
  f->map_w = w;
}

void remap_pass(vp_frame* f, const uint8_t* src, int src_h, int src_w, int which, int border, uint8_t* dst, int out_h, int out_w) {
  vp::FrameRemapParams q{};
  q.src = src;
  q.src_pitch = vp::frame_bgr_pitch(src_w);
  q.src_h = src_h;
  q.src_w = src_w;
  q.map = f->d_map[which];
  q.map_pitch = vp::frame_remap_map_pitch(out_w);
  q.border = border;
  q.dst = dst;
  q.dst_pitch = vp::frame_bgr_pitch(out_w);
  q.out_h = out_h;
  q.out_w = out_w;
  VP_HIP_CHECK(vp::launch_frame_remap(q, f->stream));
}

// ahead of every upload: the image is about to be overwritten, so the frame's stream falls in behind every consumer copy queued so far; a buffer that
// has to grow is freed only once those copies and the frame's own work have run (the one host wait of this path, once per geometry).  With
// rectification on, the picture buffer is sized by the setting's output, the raw-sized buffers by (h, w), and the maps are built here (once per
// geometry and setting, ensure_rectify_maps).
void begin_upload(vp_frame* f, int h, int w, size_t src_bytes, size_t stage_bytes) {
  f->wait_for_consumers();
  const RectifyPlan plan = rectify_plan(f, h, w);
  const size_t bgr_bytes = (size_t)plan.out_h * vp::frame_bgr_pitch(plan.out_w);
  const size_t raw_bytes = plan.on ? (size_t)h * vp::frame_bgr_pitch(w) : 0, mid_bytes = plan.pass[0] && plan.pass[1] ? raw_bytes : 0;
  if (plan.on) ensure_rectify_maps(f, plan, h, w);
  if (bgr_bytes > f->bgr_cap || raw_bytes > f->raw_cap || mid_bytes > f->mid_cap || src_bytes > f->src_cap || stage_bytes > f->stage_cap) {
    VP_HIP_CHECK(hipStreamSynchronize(f->stream));
    grow(f->d_bgr, f->bgr_cap, bgr_bytes, false);
    grow(f->d_raw, f->raw_cap, raw_bytes, false);
    grow(f->d_mid, f->mid_cap, mid_bytes, false);
    grow(f->d_src, f->src_cap, src_bytes, false);
    if (stage_bytes > f->stage_cap) {
      if (f->h_stage) (void)hipHostFree(f->h_stage);
      f->h_stage = nullptr;
      f->stage_cap = 0;
      const size_t n = (stage_bytes + 255) & ~(size_t)255;
      VP_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&f->h_stage), 2 * n, hipHostMallocDefault));   // two slots: frame n + 1 is staged while n flies
      f->stage_cap = n;
    }
  }
}

// behind the conversion of an h x w frame: the rectification passes, if any, on the frame's stream; then "content ready"
void end_upload(vp_frame* f, int h, int w) {
  const RectifyPlan plan = rectify_plan(f, h, w);
  if (plan.pass[0] && plan.pass[1]) {
    remap_pass(f, f->d_raw, h, w, 0, VP_BORDER_CONSTANT, f->d_mid, h, w);
    remap_pass(f, f->d_mid, h, w, 1, VP_BORDER_REPLICATE, f->d_bgr, plan.out_h, plan.out_w);
  } else if (plan.pass[0]) {
    remap_pass(f, f->d_raw, h, w, 0, VP_BORDER_CONSTANT, f->d_bgr, plan.out_h, plan.out_w);
  } else if (plan.pass[1]) {
    remap_pass(f, f->d_raw, h, w, 1, VP_BORDER_REPLICATE, f->d_bgr, plan.out_h, plan.out_w);
  }
  VP_HIP_CHECK(hipEventRecord(f->ready, f->stream));
  f->h = plan.out_h;
  f->w = plan.out_w;
  f->pitch = vp::frame_bgr_pitch(plan.out_w);
  f->uploaded = true;
}

// planes / strides in the format's own order, device memory
void convert_planes(vp_frame* f, int format, const uint8_t* const* p, const int* s, int n, int h, int w) {
  if (vp::frame_format_bayer(format)) {
    const vp_raw& r = f->raw;
    const int order = (format - VP_FRAME_BAYER_RGGB8) & 3;   // RGGB, GRBG, GBRG, BGGR
    vp::FrameRawParams q{};
    q.src = p[0];
    q.stride = s[0];
    q.h = h;
    q.w = w;
    q.wide = vp::frame_format_bayer16(format) ? 1 : 0;
    q.green00 = order == 1 || order == 2;
    q.red_row0 = order < 2;
    q.bits = raw_significant_bits("vp_frame_upload", f, format);
    q.shift = r.shift;
    q.black = r.black;
    std::copy(r.gains, r.gains + 3, q.gains);
    q.ccm_on = r.ccm_on ? 1 : 0;
    std::copy(r.ccm, r.ccm + 9, q.ccm);
    q.lut = r.lut_len ? f->d_lut : nullptr;
    q.dst = conversion_target(f, h, w);
    q.dst_pitch = vp::frame_bgr_pitch(w);
    VP_HIP_CHECK(vp::launch_frame_raw_to_bgr8(q, f->stream));
    return;
  }
  if (vp::frame_format_deep(format)) {
    vp::FrameDeepParams q{};
    q.p0 = p[0];
    q.s0 = s[0];
    q.p1 = n > 1 ? p[1] : nullptr;
    q.s1 = n > 1 ? s[1] : 0;
    q.h = h;
    q.w = w;
    q.format = format;
    q.dst = conversion_target(f, h, w);
    q.dst_pitch = vp::frame_bgr_pitch(w);
    q.k = vp::color_standard(f->color_matrix, f->color_range).inv;
    VP_HIP_CHECK(vp::launch_frame_deep_to_bgr8(q, f->stream));
    return;
  }
  vp::FrameToBgrParams q{};
  q.p0 = p[0];
  q.s0 = s[0];
  q.p1 = n > 1 ? p[1] : nullptr;
  q.s1 = n > 1 ? s[1] : 0;
  q.p2 = n > 2 ? p[2] : nullptr;
  q.s2 = n > 2 ? s[2] : 0;
  q.h = h;
  q.w = w;
  q.format = format;
  q.dst = conversion_target(f, h, w);
  q.dst_pitch = vp::frame_bgr_pitch(w);
  q.k = vp::color_standard(f->color_matrix, f->color_range).inv;
  VP_HIP_CHECK(vp::launch_frame_to_bgr8(q, f->stream));
}

}  // namespace

extern "C" {

int vp_frame_create(vp_frame** out, int gpu_id, char* err, size_t err_len) {
  if (!out) return VP_ERR_ARG;
  *out = nullptr;
  try {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) throw std::runtime_error("HIP error: no HIP device visible: a vp_frame lives on the device");
    if (gpu_id < 0 || gpu_id >= n) throw std::invalid_argument("gpu_id out of range");
    auto f = std::make_unique<vp_frame>();
    f->gpu = gpu_id;
    VP_HIP_CHECK(hipSetDevice(gpu_id));
    VP_HIP_CHECK(hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking));
    VP_HIP_CHECK(hipEventCreateWithFlags(&f->ready, hipEventDisableTiming));
    VP_HIP_CHECK(hipEventCreateWithFlags(&f->producer, hipEventDisableTiming));
    for (hipEvent_t& ev : f->stage_ev) VP_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    *out = f.release();
    return VP_OK;
  } catch (const std::invalid_argument& ex) {
    set_err(err, err_len, ex.what());
    return VP_ERR_ARG;
  } catch (const std::exception& ex) {
    set_err(err, err_len, ex.what());
    return VP_ERR_HIP;
  }
}

void vp_frame_destroy(vp_frame* f) { delete f; }

const char* vp_frame_last_error(const vp_frame* f) { return f ? f->err.c_str() : "null frame"; }

int vp_frame_upload(vp_frame* f, int format, const uint8_t* const* planes, const int* strides, int n_planes, int h, int w) {
  return frame_guarded(f, [&] {
    const FramePlanes fp = check_upload("vp_frame_upload", f, format, reinterpret_cast<const void* const*>(planes), strides, n_planes, h, w);
    size_t total = 0;
    bool registered = true;   // every plane inside a vp_register_frames range: one DMA per plane straight from the caller's memory
    for (int i = 0; i < fp.n; ++i) {
      total += fp.row_bytes[i] * fp.rows[i];
      registered = registered && vp::frame_range_registered(planes[i], (size_t)(fp.rows[i] - 1) * strides[i] + fp.row_bytes[i]);
    }
    const bool bgr = format == VP_FRAME_BGR8;
    begin_upload(f, h, w, bgr ? 0 : total, registered ? 0 : total);
    const int pitch = vp::frame_bgr_pitch(w);
    uint8_t* const image = conversion_target(f, h, w);   // the picture, or the raw-sized buffer ahead of the rectification passes
    if (registered) {
      size_t off = 0;
      for (int i = 0; i < fp.n; ++i) {
        uint8_t* dst = bgr ? image : f->d_src + off;
        VP_HIP_CHECK(hipMemcpy2DAsync(dst, bgr ? (size_t)pitch : fp.row_bytes[i], planes[i], strides[i], fp.row_bytes[i], fp.rows[i], hipMemcpyHostToDevice, f->stream));
        off += fp.row_bytes[i] * fp.rows[i];
      }
    } else {
      f->stage_slot ^= 1;
      uint8_t* slot = f->h_stage + (size_t)f->stage_slot * f->stage_cap;
      // the H2D that last read this slot (two uploads ago) may still be queued: its event orders this host write behind it
      VP_HIP_CHECK(hipEventSynchronize(f->stage_ev[f->stage_slot]));
      uint8_t* o = slot;
      for (int i = 0; i < fp.n; ++i)
        for (int y = 0; y < fp.rows[i]; ++y, o += fp.row_bytes[i]) std::memcpy(o, planes[i] + (size_t)y * strides[i], fp.row_bytes[i]);
      if (bgr) VP_HIP_CHECK(hipMemcpy2DAsync(image, pitch, slot, fp.row_bytes[0], fp.row_bytes[0], h, hipMemcpyHostToDevice, f->stream));
      else VP_HIP_CHECK(hipMemcpyAsync(f->d_src, slot, total, hipMemcpyHostToDevice, f->stream));
      VP_HIP_CHECK(hipEventRecord(f->stage_ev[f->stage_slot], f->stream));
    }
    if (!bgr) {   // d_src: rows packed, plane after plane
      const uint8_t* dp[3] = {f->d_src, nullptr, nullptr};
      int ds[3] = {0, 0, 0};
      for (int i = 0; i < fp.n; ++i) {
        ds[i] = (int)fp.row_bytes[i];
        if (i + 1 < fp.n) dp[i + 1] = dp[i] + fp.row_bytes[i] * fp.rows[i];
      }
      convert_planes(f, format, dp, ds, fp.n, h, w);
    }
    end_upload(f, h, w);
  });
}

int vp_frame_upload_device(vp_frame* f, int format, const void* const* dev_planes, const int* strides, int n_planes, int h, int w, void* producer_stream) {
  return frame_guarded(f, [&] {
    const FramePlanes fp = check_upload("vp_frame_upload_device", f, format, dev_planes, strides, n_planes, h, w);
    begin_upload(f, h, w, 0, 0);
    if (producer_stream) {   // the planes are complete once the work queued on the producer's stream so far has run
      VP_HIP_CHECK(hipEventRecord(f->producer, static_cast<hipStream_t>(producer_stream)));
      VP_HIP_CHECK(hipStreamWaitEvent(f->stream, f->producer, 0));
    }
    if (format == VP_FRAME_BGR8)
      VP_HIP_CHECK(hipMemcpy2DAsync(conversion_target(f, h, w), vp::frame_bgr_pitch(w), dev_planes[0], strides[0], fp.row_bytes[0], h, hipMemcpyDeviceToDevice, f->stream));
    else
      convert_planes(f, format, reinterpret_cast<const uint8_t* const*>(dev_planes), strides, fp.n, h, w);
    end_upload(f, h, w);
  });
}

int vp_frame_set_color(vp_frame* f, int matrix, int range) {
  return frame_guarded(f, [&] {
    check_color("vp_frame_set_color", matrix, range);
    f->color_matrix = matrix;
    f->color_range = range;
  });
}

int vp_frame_get_color(const vp_frame* f, int* matrix, int* range) {
  if (!f || !matrix || !range) return VP_ERR_ARG;
  *matrix = f->color_matrix;
  *range = f->color_range;
  return VP_OK;
}

int vp_frame_set_raw(vp_frame* f, const vp_raw* r) {
  return frame_guarded(f, [&] {
    const std::string me = "vp_frame_set_raw";
    vp_raw s{0, 0, 0, {256, 256, 256}, 0, {0, 0, 0, 0, 0, 0, 0, 0, 0}, nullptr, 0};
    if (r) s = *r;
    if (s.bits != 0 && s.bits != 8 && s.bits != 10 && s.bits != 12 && s.bits != 14 && s.bits != 16)
      throw std::invalid_argument(me + ": bits = " + std::to_string(s.bits) + " (0, 8, 10, 12, 14 or 16)");
    if (s.shift < 0 || s.shift > 8) throw std::invalid_argument(me + ": shift = " + std::to_string(s.shift) + " (0 .. 8)");
    if (s.black < 0) throw std::invalid_argument(me + ": black = " + std::to_string(s.black) + " is negative");
    for (int g : s.gains)
      if (g < 0 || g > 16383) throw std::invalid_argument(me + ": gain " + std::to_string(g) + " (Q8, 0 .. 16383)");
    if (s.ccm_on)
      for (int c : s.ccm)
        if (c < -8191 || c > 8191) throw std::invalid_argument(me + ": ccm entry " + std::to_string(c) + " (Q10, -8191 .. 8191)");
    if ((s.lut != nullptr) != (s.lut_len != 0)) throw std::invalid_argument(me + ": lut and lut_len go together (one is set, the other is not)");
    if (s.lut && s.lut_len != 256 && s.lut_len != 1024 && s.lut_len != 4096)
      throw std::invalid_argument(me + ": lut_len = " + std::to_string(s.lut_len) + " (256, 1024 or 4096)");
    if (s.lut) {   // ordered like the rectification maps: behind every conversion queued so far, and copied before the call returns
      VP_HIP_CHECK(hipStreamSynchronize(f->stream));
      if (!f->d_lut) VP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&f->d_lut), 4096));
      VP_HIP_CHECK(hipMemcpyAsync(f->d_lut, s.lut, (size_t)s.lut_len, hipMemcpyHostToDevice, f->stream));
      VP_HIP_CHECK(hipStreamSynchronize(f->stream));
    }
    s.ccm_on = s.ccm_on ? 1 : 0;
    s.lut = nullptr;
    f->raw = s;
  });
}

int vp_frame_get_raw(const vp_frame* f, vp_raw* out) {
  if (!f || !out) return VP_ERR_ARG;
  *out = f->raw;
  return VP_OK;
}

int vp_frame_set_rectify(vp_frame* f, const vp_rectify* r) {
  return frame_guarded(f, [&] {
    if (r) check_rectify("vp_frame_set_rectify", *r);
    f->rect_on = r != nullptr;
    if (r) f->rect = *r;
    f->map_h = f->map_w = 0;   // the next upload builds the maps of the new setting
  });
}

int vp_frame_get_rectify(const vp_frame* f, vp_rectify* out) {
  if (!f || !out) return VP_ERR_ARG;
  if (!f->rect_on) return VP_ERR_STATE;
  *out = f->rect;
  return VP_OK;
}

int vp_rectify_map(const vp_rectify* r, int src_h, int src_w, int which, int16_t* xy, uint16_t* frac) {
  try {
    if (!r || !xy || !frac || which < 0 || which > 2) return VP_ERR_ARG;
    check_rectify("vp_rectify_map", *r);
    check_rectify_source("vp_rectify_map", src_h, src_w);
    const int mh = which == 0 ? src_h : r->out_h, mw = which == 0 ? src_w : r->out_w;
    std::vector<vp::RemapEntry> m((size_t)mh * mw);
    build_rectify_map(*r, src_h, src_w, which, m.data(), mw);
    for (size_t i = 0; i < m.size(); ++i) {
      xy[2 * i] = (int16_t)(m[i].x >> 5);
      xy[2 * i + 1] = (int16_t)(m[i].y >> 5);
      frac[i] = (uint16_t)(((m[i].y & 31) << 5) | (m[i].x & 31));
    }
    return VP_OK;
  } catch (const std::invalid_argument&) {
    return VP_ERR_ARG;
  } catch (...) {
    return VP_ERR_STATE;
  }
}

int vp_rectify_homography(const vp_camera_pose* inference, const vp_camera_pose* standard, double H_out[9]) {
  if (!inference || !standard || !H_out) return VP_ERR_ARG;
  const vp_camera_pose &pi = *inference, &ps = *standard;
  for (double v : {pi.pitch_deg, pi.yaw_deg, pi.roll_deg, pi.camera_height, ps.pitch_deg, ps.yaw_deg, ps.roll_deg, ps.camera_height, ps.hfov_deg})
    if (!std::isfinite(v)) return VP_ERR_ARG;
  for (double v : pi.K)
    if (!std::isfinite(v)) return VP_ERR_ARG;
  const double* K = pi.K;
  if (K[0] == 0.0 || K[4] == 0.0 || K[1] != 0.0 || K[3] != 0.0 || K[6] != 0.0 || K[7] != 0.0 || K[8] != 1.0) return VP_ERR_ARG;
  if (pi.camera_height == 0.0 || ps.img_w < 1 || ps.img_h < 1 || !(ps.hfov_deg > 0.0 && ps.hfov_deg < 180.0)) return VP_ERR_ARG;
  const double rad = 3.14159265358979323846 / 180.0;
  auto rodrigues = [&](const vp_camera_pose& p, double* R) {   // cos I + (1 - cos) k k^T + sin [k]x of the vector (pitch, yaw, roll)
    const double v[3] = {p.pitch_deg * rad, p.yaw_deg * rad, p.roll_deg * rad};
    const double th = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    for (int i = 0; i < 9; ++i) R[i] = i % 4 == 0 ? 1.0 : 0.0;
    if (th == 0.0) return;
    const double k[3] = {v[0] / th, v[1] / th, v[2] / th}, c = std::cos(th), s = std::sin(th);
    const double kx[9] = {0.0, -k[2], k[1], k[2], 0.0, -k[0], -k[1], k[0], 0.0};
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) R[3 * i + j] = c * (i == j ? 1.0 : 0.0) + (1.0 - c) * k[i] * k[j] + s * kx[3 * i + j];
  };
  auto mul = [](const double* A, const double* B, double* Cm) {
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) Cm[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
  };
  double Rs[9], Ri[9], RiT[9], Rrel[9], T[9];
  rodrigues(ps, Rs);
  rodrigues(pi, Ri);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) RiT[3 * i + j] = Ri[3 * j + i];
  mul(Rs, RiT, Rrel);
  const double fs = (ps.img_w / 2.0) / std::tan(ps.hfov_deg * rad / 2.0);
  const double Ks[9] = {fs, 0.0, ps.img_w / 2.0, 0.0, fs * (ps.camera_height / pi.camera_height), ps.img_h / 2.0, 0.0, 0.0, 1.0};
  const double Kinv[9] = {1.0 / K[0], 0.0, -K[2] / K[0], 0.0, 1.0 / K[4], -K[5] / K[4], 0.0, 0.0, 1.0};
  mul(Ks, Rrel, T);
  mul(T, Kinv, H_out);
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(H_out[i])) return VP_ERR_ARG;
  return VP_OK;
}

int vp_frame_sync(vp_frame* f) {
  return frame_guarded(f, [&] { VP_HIP_CHECK(hipStreamSynchronize(f->stream)); });
}

int vp_frame_dims(const vp_frame* f, int* h, int* w) {
  if (!f || !h || !w) return VP_ERR_ARG;
  if (!f->uploaded) return VP_ERR_STATE;
  *h = f->h;
  *w = f->w;
  return VP_OK;
}

int vp_frame_fetch_bgr8(vp_frame* f, uint8_t* dst, int dst_stride) {
  return frame_guarded(f, [&] {
    if (!f->uploaded) throw std::runtime_error("the frame was never uploaded (vp_frame_upload / vp_frame_upload_device first)");
    if (!dst || dst_stride < 3 * f->w) throw std::invalid_argument("vp_frame_fetch_bgr8: null destination or a stride below 3 * width");
    VP_HIP_CHECK(hipMemcpy2DAsync(dst, dst_stride, f->d_bgr, f->pitch, (size_t)3 * f->w, f->h, hipMemcpyDeviceToHost, f->stream));
    VP_HIP_CHECK(hipStreamSynchronize(f->stream));
  });
}

int vp_upload_from_frame(vp_engine* e, vp_frame* f, int x0, int y0, int w, int h) {
  return guarded(e, [&](vp::Engine& g) {
    if (!f) throw std::invalid_argument("null frame");
    g.upload_from_frame(f->view(), x0, y0, w, h);
    f->note_consumer(g.stream());   // the next upload into the frame waits for this copy, on the device
  });
}

int vp_infer_frame(vp_engine* e, vp_frame* f, int x0, int y0, int w, int h) {
  return guarded(e, [&](vp::Engine& g) {
    if (!f) throw std::invalid_argument("null frame");
    g.upload_from_frame(f->view(), x0, y0, w, h);
    f->note_consumer(g.stream());
    g.enqueue();
    g.fetch_outputs();
  });
}

// ---- vp_canvas: one picture per camera frame (include/vp_hip.h; vp::Canvas: engine.hpp / engine_io.cpp; kernels: kernels_misc.hip canvas_*)
}  // extern "C"

namespace {

template <class F>
int canvas_guarded(vp_canvas* c, F&& fn) {
  if (!c || !c->impl) return VP_ERR_ARG;
  try {
    fn(*c->impl);
    return VP_OK;
  } catch (const std::invalid_argument& ex) {
    c->err = ex.what();
    return VP_ERR_ARG;
  } catch (const std::exception& ex) {
    c->err = ex.what();
    return std::strncmp(ex.what(), "HIP error", 9) == 0 ? VP_ERR_HIP : VP_ERR_STATE;
  }
}

// drawUntrackedDetection's rectangle (autospeed_visualization_engine.cpp:131-132) and getColorByClass's colour: float subtraction, truncation toward
// zero; false: nothing to draw.  Coordinates the int conversion cannot hold (a detector clamps to the frame: never its output) are refused by the caller.
bool detection_box(const vp_detection& d, vp::CanvasBox* b) {
  const int bx = (int)d.x1, by = (int)d.y1, bw = (int)(d.x2 - d.x1), bh = (int)(d.y2 - d.y1);
  if (bw <= 0 || bh <= 0) return false;
  b->x0 = bx;
  b->y0 = by;
  b->x1 = bx + bw - 1;
  b->y1 = by + bh - 1;
  b->bgr = d.class_id == 1 ? 0xFF0000u : d.class_id == 2 ? 0xFFFF00u : d.class_id == 3 ? 0x00FFFFu : 0xFFFFFFu;   // b | g << 8 | r << 16
  return true;
}

}  // namespace

extern "C" {

int vp_canvas_create(vp_canvas** out, int gpu_id, char* err, size_t err_len) {
  if (!out) return VP_ERR_ARG;
  *out = nullptr;
  try {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) throw std::runtime_error("HIP error: no HIP device visible: a vp_canvas lives on the device");
    if (gpu_id < 0 || gpu_id >= n) throw std::invalid_argument("gpu_id out of range");
    auto c = std::make_unique<vp_canvas>();
    c->impl = std::make_unique<vp::Canvas>(gpu_id);
    *out = c.release();
    return VP_OK;
  } catch (const std::invalid_argument& ex) {
    set_err(err, err_len, ex.what());
    return VP_ERR_ARG;
  } catch (const std::exception& ex) {
    set_err(err, err_len, ex.what());
    return VP_ERR_HIP;
  }
}

void vp_canvas_destroy(vp_canvas* c) { delete c; }

const char* vp_canvas_last_error(const vp_canvas* c) { return c ? c->err.c_str() : "null canvas"; }

int vp_canvas_begin(vp_canvas* c, vp_frame* f) {
  return canvas_guarded(c, [&](vp::Canvas& g) {
    if (!f) throw std::invalid_argument("vp_canvas_begin: null frame");
    g.begin(f->view());
    f->note_consumer(g.stream());   // the next upload into the frame waits for this copy, on the device
  });
}

int vp_canvas_blend_mask(vp_canvas* c, vp_engine* e, int viz_type) {
  return canvas_guarded(c, [&](vp::Canvas& g) {
    if (!e || !e->impl) throw std::invalid_argument("vp_canvas_blend_mask: null engine");
    g.blend_mask(*e->impl, viz_type);
  });
}

int vp_canvas_blend_mask_u8(vp_canvas* c, const uint8_t* mask, int mask_on_device, int mh, int mw, int viz_type, int x0, int y0, int w, int h) {
  return canvas_guarded(c, [&](vp::Canvas& g) { g.blend_mask_u8(mask, mask_on_device != 0, mh, mw, viz_type, x0, y0, w, h); });
}

int vp_canvas_paste_depth(vp_canvas* c, vp_engine* e) {
  return canvas_guarded(c, [&](vp::Canvas& g) {
    if (!e || !e->impl) throw std::invalid_argument("vp_canvas_paste_depth: null engine");
    g.paste_depth(*e->impl);
  });
}

int vp_canvas_draw_detections(vp_canvas* c, const vp_detection* dets, int n) {
  return canvas_guarded(c, [&](vp::Canvas& g) {
    if (n < 0 || (n > 0 && !dets)) throw std::invalid_argument("vp_canvas_draw_detections: n < 0, or null detections with n > 0");
    std::vector<vp::CanvasBox> boxes;
    boxes.reserve((size_t)n);
    for (int i = 0; i < n; ++i) {
      const vp_detection& d = dets[i];
      for (float v : {d.x1, d.y1, d.x2, d.y2})
        if (!(v > -1e8f && v < 1e8f)) throw std::invalid_argument("vp_canvas_draw_detections: detection " + std::to_string(i) + " has a coordinate that is not a pixel position");
      vp::CanvasBox b;
      if (detection_box(d, &b)) boxes.push_back(b);
    }
    g.draw_boxes(boxes.data(), (int)boxes.size());
  });
}

int vp_canvas_sync(vp_canvas* c) {
  return canvas_guarded(c, [&](vp::Canvas& g) { g.sync(); });
}

int vp_canvas_dims(const vp_canvas* c, int* h, int* w) {
  if (!c || !c->impl || !h || !w) return VP_ERR_ARG;
  if (!c->impl->begun()) return VP_ERR_STATE;
  *h = c->impl->h();
  *w = c->impl->w();
  return VP_OK;
}

int vp_canvas_device(const vp_canvas* c, void** dev_bgr8, int* pitch_bytes) {
  if (!c || !c->impl || !dev_bgr8 || !pitch_bytes) return VP_ERR_ARG;
  if (!c->impl->begun()) return VP_ERR_STATE;
  *dev_bgr8 = c->impl->device();
  *pitch_bytes = c->impl->pitch();
  return VP_OK;
}

int vp_canvas_layout3(int format, int h, int w, int* n_planes, int row_bytes[3], int rows[3]) {
  if (!n_planes || !row_bytes || !rows) return VP_ERR_ARG;
  try {
    const FramePlanes fp = frame_layout("vp_canvas_layout3", format, h, w);
    *n_planes = fp.n;
    for (int i = 0; i < 3; ++i) {
      row_bytes[i] = (int)fp.row_bytes[i];
      rows[i] = fp.rows[i];
    }
    return VP_OK;
  } catch (const std::exception&) {
    return VP_ERR_ARG;
  }
}

int vp_canvas_layout(int format, int h, int w, int* n_planes, int row_bytes[2], int rows[2]) {
  if (!n_planes || !row_bytes || !rows || format_planes(format) > 2) return VP_ERR_ARG;   // the three-plane formats: vp_canvas_layout3
  int rb[3], rw[3];
  const int rc = vp_canvas_layout3(format, h, w, n_planes, rb, rw);
  if (rc != VP_OK) return rc;
  for (int i = 0; i < 2; ++i) {
    row_bytes[i] = rb[i];
    rows[i] = rw[i];
  }
  return VP_OK;
}

int vp_canvas_set_color(vp_canvas* c, int matrix, int range, int chroma_mode) {
  return canvas_guarded(c, [&](vp::Canvas& g) {
    check_color("vp_canvas_set_color", matrix, range);
    if (chroma_mode != VP_CHROMA_EVEN && chroma_mode != VP_CHROMA_MEAN)
      throw std::invalid_argument("vp_canvas_set_color: unknown chroma mode " + std::to_string(chroma_mode) + " (VP_CHROMA_EVEN, VP_CHROMA_MEAN)");
    g.set_color(matrix, range, chroma_mode);
  });
}

int vp_canvas_get_color(const vp_canvas* c, int* matrix, int* range, int* chroma_mode) {
  if (!c || !c->impl || !matrix || !range || !chroma_mode) return VP_ERR_ARG;
  c->impl->get_color(matrix, range, chroma_mode);
  return VP_OK;
}

int vp_canvas_fetch(vp_canvas* c, int format, uint8_t* const* planes, const int* strides, int n_planes) {
  return canvas_guarded(c, [&](vp::Canvas& g) {
    if (!g.begun()) throw std::runtime_error("vp_canvas_fetch: the canvas holds no picture (vp_canvas_begin first)");
    const FramePlanes fp = check_frame_planes("vp_canvas_fetch", format, reinterpret_cast<const void* const*>(planes), strides, n_planes, g.h(), g.w());
    g.fetch(format, planes, strides, fp.row_bytes, fp.rows, fp.n);
  });
}

int vp_canvas_add_planes_f32(vp_canvas* c, const float* planes, int planes_on_device, int n_planes, int mh, int mw, float threshold, const uint8_t* add_bgr, int x0,
                             int y0, int w, int h) {
  return canvas_guarded(c, [&](vp::Canvas& g) { g.add_planes(planes, planes_on_device != 0, n_planes, mh, mw, threshold, add_bgr, x0, y0, w, h); });
}

int vp_canvas_overlay_lanes(vp_canvas* c, vp_engine* e, float threshold) {
  return canvas_guarded(c, [&](vp::Canvas& g) {
    if (!e || !e->impl) throw std::invalid_argument("vp_canvas_overlay_lanes: null engine");
    g.overlay_lanes(*e->impl, threshold);
  });
}

int vp_canvas_draw_points(vp_canvas* c, const int* xy, int n, int radius, const uint8_t* bgr) {
  return canvas_guarded(c, [&](vp::Canvas& g) {
    if (n < 0 || n > 4096 || (n > 0 && !xy)) throw std::invalid_argument("vp_canvas_draw_points: n outside 0 .. 4096, or null points with n > 0");
    if (radius < 0 || radius > vp::kCanvasMaxRadius) throw std::invalid_argument("vp_canvas_draw_points: radius " + std::to_string(radius) + " (0 .. 16)");
    if (!bgr) throw std::invalid_argument("vp_canvas_draw_points: null colour");
    g.draw_points(xy, n, radius, (unsigned)bgr[0] | ((unsigned)bgr[1] << 8) | ((unsigned)bgr[2] << 16));
  });
}

int vp_canvas_draw_lane_rows(vp_canvas* c, vp_engine* e) {
  return canvas_guarded(c, [&](vp::Canvas& g) {
    if (!e || !e->impl) throw std::invalid_argument("vp_canvas_draw_lane_rows: null engine");
    g.draw_lane_rows(*e->impl);
  });
}

int vp_canvas_fetch_resized(vp_canvas* c, int format, int out_h, int out_w, uint8_t* const* planes, const int* strides, int n_planes) {
  return canvas_guarded(c, [&](vp::Canvas& g) {
    if (!g.begun()) throw std::runtime_error("vp_canvas_fetch_resized: the canvas holds no picture (vp_canvas_begin first)");
    const FramePlanes fp = check_frame_planes("vp_canvas_fetch_resized", format, reinterpret_cast<const void* const*>(planes), strides, n_planes, out_h, out_w, 1);
    g.fetch_resized(format, out_h, out_w, planes, strides, fp.row_bytes, fp.rows, fp.n);
  });
}

// the refusals every JPEG entry shares: the geometry's are the I420 fetch's own, with its texts
static void check_jpeg_args(const char* who, int h, int w, int quality, int restart_mcus) {
  const std::string me(who);
  if (quality < 1 || quality > 100) throw std::invalid_argument(me + ": quality " + std::to_string(quality) + " (1 .. 100)");
  if (restart_mcus < 0 || restart_mcus > 65535)
    throw std::invalid_argument(me + ": restart_mcus " + std::to_string(restart_mcus) + " (1 .. 65535, or 0 for the default " + std::to_string(vp::kJpegDefaultRestart) + ")");
  (void)frame_layout(me, VP_FRAME_I420, h, w);
}

int vp_canvas_fetch_jpeg(vp_canvas* c, int quality, int restart_mcus, uint8_t* dst, size_t cap, size_t* n) {
  return canvas_guarded(c, [&](vp::Canvas& g) {
    if (!dst || !n) throw std::invalid_argument("vp_canvas_fetch_jpeg: null dst / n");
    if (!g.begun()) throw std::runtime_error("vp_canvas_fetch_jpeg: the canvas holds no picture (vp_canvas_begin first)");
    check_jpeg_args("vp_canvas_fetch_jpeg", g.h(), g.w(), quality, restart_mcus);
    g.fetch_jpeg(0, 0, quality, restart_mcus, dst, cap, n);
  });
}

int vp_canvas_fetch_jpeg_resized(vp_canvas* c, int out_h, int out_w, int quality, int restart_mcus, uint8_t* dst, size_t cap, size_t* n) {
  return canvas_guarded(c, [&](vp::Canvas& g) {
    if (!dst || !n) throw std::invalid_argument("vp_canvas_fetch_jpeg_resized: null dst / n");
    if (!g.begun()) throw std::runtime_error("vp_canvas_fetch_jpeg_resized: the canvas holds no picture (vp_canvas_begin first)");
    check_jpeg_args("vp_canvas_fetch_jpeg_resized", out_h, out_w, quality, restart_mcus);
    g.fetch_jpeg(out_h, out_w, quality, restart_mcus, dst, cap, n);
  });
}

int vp_sync(vp_engine* e) {
  return guarded(e, [&](vp::Engine& g) { g.sync(); });
}
int vp_fetch_outputs(vp_engine* e) {
  return guarded(e, [&](vp::Engine& g) { g.fetch_outputs(); });
}
int vp_device_outputs(const vp_engine* e, void** logits, void** mask) {
  if (!e || !e->impl) return VP_ERR_ARG;
  if (logits) *logits = e->impl->dev_logits();
  if (mask) *mask = e->impl->dev_mask();
  return VP_OK;
}
int vp_use_graph(vp_engine* e, int enable) {
  return guarded(e, [&](vp::Engine& g) { g.use_graph(enable != 0); });
}
int vp_timer_begin(vp_engine* e) {
  return guarded(e, [&](vp::Engine& g) { g.timer_begin(); });
}
int vp_timer_end(vp_engine* e, float* ms) {
  return guarded(e, [&](vp::Engine& g) {
    const float t = g.timer_end();
    if (ms) *ms = t;
  });
}

int vp_layer_count(const vp_engine* e) { return (e && e->impl) ? (int)e->impl->ops().size() : VP_ERR_ARG; }
int vp_layer_info(const vp_engine* e, int i, const char** name, double* flops, double* bytes) {
  if (!e || !e->impl || i < 0 || i >= (int)e->impl->ops().size()) return VP_ERR_ARG;
  const vp::Op& op = e->impl->ops()[i];
  if (name) *name = op.name.c_str();
  if (flops) *flops = op.flops;
  if (bytes) *bytes = op.bytes;
  return VP_OK;
}
int vp_layer_flops_executed(const vp_engine* e, int i, double* flops) {
  if (!e || !e->impl || !flops || i < 0 || i >= (int)e->impl->ops().size()) return VP_ERR_ARG;
  const vp::Op& op = e->impl->ops()[i];
  *flops = op.flops_executed > 0 ? op.flops_executed : op.flops;
  return VP_OK;
}
int vp_layer_kernel(const vp_engine* e, int i, const char** kernel) {
  if (!e || !e->impl || !kernel || i < 0 || i >= (int)e->impl->ops().size()) return VP_ERR_ARG;
  *kernel = e->impl->ops()[i].kernel.c_str();
  return VP_OK;
}
// AutoSteerOnnxEngine::postProcess (production_release/src/inference/autosteer_engine.cpp:160-185): first maximum wins, angle = class - 30
float vp_autosteer_angle(const float* logits, int classes) {
  if (!logits || classes < 1) return 0.0f;
  int best = 0;
  float best_v = logits[0];
  for (int i = 1; i < classes; ++i)
    if (logits[i] > best_v) {
      best_v = logits[i];
      best = i;
    }
  return static_cast<float>(best - 30);
}
// launch geometry beyond the tag ("nsplit=4", "groups=32", "nsplit=2 wgs=128"; "" when the tag says it all): what vp_plan_hash mixes in third
int vp_layer_launch(const vp_engine* e, int i, const char** launch) {
  if (!e || !e->impl || !launch || i < 0 || i >= (int)e->impl->ops().size()) return VP_ERR_ARG;
  *launch = e->impl->ops()[i].launch.c_str();
  return VP_OK;
}
// FNV-1a over (launch name, kernel tag, launch geometry) of every launch of the plan: two engines with equal hashes run the same kernels with the same
// split factors / group counts in the same order
unsigned long long vp_plan_hash(const vp_engine* e) {
  if (!e || !e->impl) return 0;
  unsigned long long h = 1469598103934665603ull;
  auto mix = [&h](const std::string& t) {
    for (unsigned char c : t) {
      h ^= c;
      h *= 1099511628211ull;
    }
    h ^= 0xffu;
    h *= 1099511628211ull;
  };
  for (const vp::Op& op : e->impl->ops()) {
    mix(op.name);
    mix(op.kernel);
    if (!op.launch.empty()) mix(op.launch);
  }
  return h ? h : 1;
}
int vp_weight_bytes(const vp_engine* e, unsigned long long* fp8_bytes, unsigned long long* fp16_bytes, unsigned long long* fp32_bytes) {
  if (!e || !e->impl) return VP_ERR_ARG;
  const unsigned long long* w = e->impl->weight_bytes();
  if (fp8_bytes) *fp8_bytes = w[0];
  if (fp16_bytes) *fp16_bytes = w[1];
  if (fp32_bytes) *fp32_bytes = w[2];
  return VP_OK;
}
// host only: the (hi, lo) fp16 planes and the per-row 2^-s the engine makes of a weight matrix (engine.cpp row_prescale + split_half)
int vp_split_weight_rows(const float* w, int rows, int per_row, uint16_t* hi, uint16_t* lo, float* post_scale) {
  if (!w || rows < 1 || per_row < 1 || !hi || !lo || !post_scale) return VP_ERR_ARG;
  try {
    const vp::RowScale rs = vp::row_prescale(w, (size_t)rows, (size_t)per_row, (size_t)rows);
    for (int r = 0; r < rows; ++r) {
      post_scale[r] = rs.post[r];
      for (int i = 0; i < per_row; ++i) {
        vp::half_t h, l;
        vp::split_half(w[(size_t)r * per_row + i], rs.pre[r], &h, &l);
        std::memcpy(hi + (size_t)r * per_row + i, &h, 2);
        std::memcpy(lo + (size_t)r * per_row + i, &l, 2);
      }
    }
  } catch (const vp::RangeError&) {
    return VP_ERR_RANGE;
  }
  return VP_OK;
}
// host only: the e4m3 codes and row scales VP_WEIGHTS_FP8 storage makes of a (quantised, possibly re-scaled) weight matrix
int vp_fp8_encode_rows(const float* w, int rows, int per_row, uint8_t* codes, float* row_scale) {
  if (!w || rows < 1 || per_row < 1 || !codes || !row_scale) return VP_ERR_ARG;
  for (int r = 0; r < rows; ++r) {
    float amax = 0.0f;
    for (int i = 0; i < per_row; ++i) amax = std::max(amax, std::fabs(w[(size_t)r * per_row + i]));
    row_scale[r] = vp::fp8_row_scale(amax);
    for (int i = 0; i < per_row; ++i) codes[(size_t)r * per_row + i] = vp::e4m3_encode(w[(size_t)r * per_row + i] / row_scale[r]);
  }
  return VP_OK;
}
int vp_copy_outputs_device(vp_engine* e, void* logits_dst, void* mask_dst) {
  return guarded(e, [&](vp::Engine& g) { g.copy_outputs_device(logits_dst, mask_dst); });
}
int vp_profile_layers(vp_engine* e, int iters, float* ms, int capacity) {
  int n = 0;
  const int rc = guarded(e, [&](vp::Engine& g) { n = g.profile_layers(iters, ms, capacity); });
  return rc == VP_OK ? n : rc;
}
int vp_tensor_count(const vp_engine* e) { return (e && e->impl) ? (int)e->impl->acts().size() : VP_ERR_ARG; }
int vp_tensor_info(const vp_engine* e, int i, const char** name, int* c, int* h, int* w) {
  if (!e || !e->impl || i < 0 || i >= (int)e->impl->acts().size()) return VP_ERR_ARG;
  const vp::Act& a = *e->impl->acts()[i];
  if (name) *name = a.name.c_str();
  if (c) *c = a.Creal;
  if (h) *h = a.H;
  if (w) *w = a.W;
  return VP_OK;
}
int vp_tensor_read(vp_engine* e, int i, float* dst) {
  return guarded(e, [&](vp::Engine& g) { g.read_act(i, dst); });
}

// ---- VP_ACT_SCALE: per-tensor power-of-two activation scale (engine_io.cpp)
int vp_calibrate_range(vp_engine* e, int target_log2) {
  return guarded(e, [&](vp::Engine& g) { g.calibrate_range(target_log2); });
}
int vp_reset_range(vp_engine* e) {
  return guarded(e, [&](vp::Engine& g) { g.reset_range(); });
}
int vp_act_scales(const vp_engine* e, int* exps, int cap) {
  if (!e || !e->impl || (cap > 0 && !exps)) return VP_ERR_ARG;
  const std::vector<int> v = e->impl->act_scales();
  for (int i = 0; i < cap && i < (int)v.size(); ++i) exps[i] = v[i];
  return (int)v.size();
}
int vp_set_act_scales(vp_engine* e, const int* exps, int n) {
  return guarded(e, [&](vp::Engine& g) { g.set_act_scales(exps, n); });
}

// ---- VP_MFMA_FP8: per-layer activation exponents of the e4m3 MFMA layers (engine_io.cpp)
int vp_calibrate_fp8(vp_engine* e, int target_log2) {
  return guarded(e, [&](vp::Engine& g) { g.calibrate_fp8(target_log2); });
}
int vp_reset_fp8(vp_engine* e) {
  return guarded(e, [&](vp::Engine& g) { g.reset_fp8(); });
}
int vp_fp8_layers(const vp_engine* e, vp_fp8_layer* out, int cap) {
  if (!e || !e->impl || cap < 0 || (cap > 0 && !out) || !e->impl->mfma_fp8()) return VP_ERR_ARG;
  const std::vector<vp::Engine::Fp8Layer>& v = e->impl->fp8_layers();
  for (int i = 0; i < cap && i < (int)v.size(); ++i) out[i] = vp_fp8_layer{(int)v[i].op, v[i].tensor, v[i].qexp};
  return (int)v.size();
}
int vp_set_fp8_exps(vp_engine* e, const int* exps, int n) {
  return guarded(e, [&](vp::Engine& g) { g.set_fp8_exps(exps, n); });
}
// host only: the quantiser of the e4m3 MFMA layers (common.hpp e4m3_quantize) over fp16 bit patterns
int vp_fp8_quantize_act(const uint16_t* f16, size_t n, int qexp, uint8_t* codes) {
  if ((n > 0 && (!f16 || !codes)) || qexp < -24 || qexp > 24) return VP_ERR_ARG;
  const float mul = std::ldexp(1.0f, -qexp);
  for (size_t i = 0; i < n; ++i) {
    vp::half_t h;
    std::memcpy(&h, f16 + i, 2);
    codes[i] = (uint8_t)vp::e4m3_quantize((float)h, mul);
  }
  return VP_OK;
}

// ---- range survey (engine_io.cpp Engine::range_survey)
static_assert(VP_RANGE_BINS == vp::VP_HIST_BINS && VP_RANGE_EXP_MIN == vp::VP_HIST_EXP_MIN, "vp_hip.h and kernels.hpp describe one histogram");
int vp_range_survey(vp_engine* e, vp_range_stats* out, int cap) {
  if (cap < 0 || (cap > 0 && !out)) return VP_ERR_ARG;
  int n = 0;
  const int rc = guarded(e, [&](vp::Engine& g) {
    const std::vector<vp::Engine::RangeStats> v = g.range_survey();
    n = (int)v.size();
    for (int i = 0; i < cap && i < n; ++i) {
      vp_range_stats& o = out[i];
      o.absmax = v[i].absmax;
      o.exp = v[i].exp;
      o.count = v[i].count;
      o.nonfinite = v[i].nonfinite;
      o.zeros = v[i].zeros;
      std::memcpy(o.bins, v[i].bins, sizeof(o.bins));
    }
  });
  return rc == VP_OK ? n : rc;
}

// ---- single-operator entries (unit tests launch one kernel or one add_* call through them; no host calls them)
// ---- vp_metric: the reference's validation scores on the device (include/vp_hip.h; vp::Metric: engine.hpp / engine_io.cpp; kernels: kernels_misc.hip metric_*)
}  // extern "C"

namespace {

static_assert(sizeof(vp_metric_frame) == sizeof(vp::MetricRecord) && offsetof(vp_metric_frame, nonfinite) == offsetof(vp::MetricRecord, nonfinite) &&
                  offsetof(vp_metric_frame, q_lo) == offsetof(vp::MetricRecord, q_lo) && offsetof(vp_metric_frame, mel) == offsetof(vp::MetricRecord, mel),
              "vp_metric_frame is the record the kernels write");

template <class F>
int metric_guarded(vp_metric* m, F&& fn) {
  if (!m || !m->impl) return VP_ERR_ARG;
  try {
    fn(*m->impl);
    return VP_OK;
  } catch (const std::invalid_argument& ex) {
    m->err = ex.what();
    return VP_ERR_ARG;
  } catch (const std::exception& ex) {
    m->err = ex.what();
    return std::strncmp(ex.what(), "HIP error", 9) == 0 ? VP_ERR_HIP : VP_ERR_STATE;
  }
}

vp::Engine& metric_engine(vp_engine* e, const char* who) {
  if (!e || !e->impl) throw std::invalid_argument(std::string(who) + ": null engine");
  return *e->impl;
}

// the scores of one segmentation record, in double: iou[c] = (I + 1) / (U + 1), U = P + G - I; *full over the sums
void seg_scores(const vp_metric_frame& r, int classes, double iou[3], double* full) {
  double si = 0.0, su = 0.0;
  for (int c = 0; c < classes; ++c) {
    const double i = (double)r.I[c], u = (double)r.P[c] + (double)r.G[c] - (double)r.I[c];
    iou[c] = (i + 1.0) / (u + 1.0);
    si += i;
    su += u;
  }
  *full = (si + 1.0) / (su + 1.0);
}

void metric_summary(const std::vector<vp_metric_frame>& recs, vp_metric_summary* s) {
  std::memset(s, 0, sizeof(*s));
  double iou[3] = {0, 0, 0}, full = 0, dom = 0, mae = 0, mel = 0;
  int scored = 0;
  for (const vp_metric_frame& r : recs) {
    ++s->frames;
    double f[3], ff;
    if (r.kind == VP_SCENESEG) {
      seg_scores(r, 3, f, &ff);
      for (int c = 0; c < 3; ++c) iou[c] += f[c];
      full += ff;
      ++s->sceneseg_frames;
    } else if (r.kind == VP_DOMAINSEG) {
      seg_scores(r, 1, f, &ff);
      dom += ff;
      ++s->domainseg_frames;
    } else {
      ++s->scene3d_frames;
      if (std::isnan(r.mae) || std::isnan(r.mel)) {
        ++s->nan_frames;
      } else {
        mae += (double)r.mae;
        mel += (double)r.mel;
        ++scored;
      }
    }
  }
  const double nan = std::nan("");
  for (int c = 0; c < 3; ++c) s->sceneseg_iou[c] = s->sceneseg_frames ? iou[c] / s->sceneseg_frames : nan;
  s->sceneseg_iou_full = s->sceneseg_frames ? full / s->sceneseg_frames : nan;
  s->domainseg_iou = s->domainseg_frames ? dom / s->domainseg_frames : nan;
  s->mae = scored ? mae / scored : nan;
  s->mel = scored ? mel / scored : nan;
}

// ---- the detector's dataset scores: compute_ap (Models/training/auto_speed_util.py:225-300) in double, statement for statement
static_assert(sizeof(vp_metric_det_frame) == sizeof(vp::DetFrameRecord) && sizeof(vp_metric_det_row) == sizeof(vp::DetRowRecord) && offsetof(vp_metric_det_row, tp) == offsetof(vp::DetRowRecord, tp) &&
                  offsetof(vp_metric_det_frame, first_row) == offsetof(vp::DetFrameRecord, first_row),
              "vp_metric_det_frame / vp_metric_det_row are the records the kernels write");
static_assert(VP_DET_MAX_NMS == vp::kDetValMaxNms && VP_DET_MAX_DET == vp::kDetValMaxDet && VP_DET_MAX_CLASSES == vp::kDetValMaxClasses && VP_DET_MAX_IOU == vp::kDetValMaxIou &&
                  VP_DET_MAX_LABELS == vp::kDetValMaxLabels,
              "the header's limits are the kernels'");

// numpy.interp for one x (compiled_base.c arr_interp): xp non-decreasing, j = the last index with xp[j] <= x
double np_interp(double x, const std::vector<double>& xp, const std::vector<double>& fp, double left, double right) {
  const size_t n = xp.size();
  if (n == 1) return x < xp[0] ? left : (x > xp[0] ? right : fp[0]);
  if (x > xp[n - 1]) return right;
  if (x < xp[0]) return left;
  const size_t j = (size_t)(std::upper_bound(xp.begin(), xp.end(), x) - xp.begin()) - 1;
  if (j == n - 1 || xp[j] == x) return fp[j];
  const double slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]);
  double r = slope * (x - xp[j]) + fp[j];
  if (std::isnan(r)) {
    r = slope * (x - xp[j + 1]) + fp[j + 1];
    if (std::isnan(r) && fp[j] == fp[j + 1]) r = fp[j];
  }
  return r;
}

// numpy.linspace(0, 1, num)
std::vector<double> np_linspace01(int num) {
  std::vector<double> x((size_t)num);
  const double step = 1.0 / (double)(num - 1);
  for (int i = 0; i < num; ++i) x[(size_t)i] = (double)i * step;
  x[(size_t)num - 1] = 1.0;
  return x;
}

void det_ap(const uint32_t* tp_in, const float* conf_in, const float* cls_in, int n_rows, const float* label_cls, int n_labels, int n_iou, vp_metric_det_summary* s) {
  const double eps = 1e-16;
  const int frames = s->frames;
  std::memset(s, 0, sizeof(*s));
  s->frames = frames;
  s->rows = n_rows;
  s->labels = n_labels;
  s->n_iou = n_iou;
  s->grid_index = -1;
  // unique_classes, nt = numpy.unique(target, return_counts=True)
  std::vector<float> uc(label_cls, label_cls + n_labels);
  std::sort(uc.begin(), uc.end());
  std::vector<double> nt;
  {
    std::vector<float> u;
    for (float v : uc) {
      if (u.empty() || u.back() != v) {
        u.push_back(v);
        nt.push_back(0.0);
      }
      nt.back() += 1.0;
    }
    uc.swap(u);
  }
  const int nc = (int)uc.size();
  s->classes = nc;
  for (int ci = 0; ci < nc && ci < VP_DET_MAX_CLASSES; ++ci) {
    s->class_id[ci] = uc[(size_t)ci];
    s->class_labels[ci] = (uint32_t)nt[(size_t)ci];
  }
  const uint32_t mask = n_iou >= 32 ? 0xFFFFFFFFu : (1u << n_iou) - 1u;
  bool any = false;
  for (int i = 0; i < n_rows; ++i) any = any || (tp_in[i] & mask) != 0;
  if (!any || nc == 0) return;   // the trainer's `metrics[0].any()`: the scores stay 0
  // i = numpy.argsort(-conf)
  std::vector<int> order((size_t)n_rows);
  for (int i = 0; i < n_rows; ++i) order[(size_t)i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return -conf_in[a] < -conf_in[b]; });
  const std::vector<double> px = np_linspace01(1000), x101 = np_linspace01(101);
  std::vector<std::vector<double>> p((size_t)nc, std::vector<double>(1000, 0.0)), r((size_t)nc, std::vector<double>(1000, 0.0)), ap((size_t)nc, std::vector<double>((size_t)n_iou, 0.0));
  for (int ci = 0; ci < nc; ++ci) {
    std::vector<int> idx;
    for (int k : order)
      if (cls_in[k] == uc[(size_t)ci]) idx.push_back(k);
    const double nl = nt[(size_t)ci];
    const size_t no = idx.size();
    if (no == 0 || nl == 0.0) continue;
    std::vector<double> neg_conf(no);
    for (size_t k = 0; k < no; ++k) neg_conf[k] = (double)(-conf_in[idx[k]]);
    std::vector<double> recall(no), precision(no), m_rec(no + 2), m_pre(no + 2), y(101);
    for (int j = 0; j < n_iou; ++j) {
      long long tpc = 0, fpc = 0;
      for (size_t k = 0; k < no; ++k) {
        const int t = (int)((tp_in[idx[k]] >> j) & 1u);
        tpc += t;
        fpc += 1 - t;
        recall[k] = (double)tpc / (nl + eps);
        precision[k] = (double)tpc / (double)(tpc + fpc);
      }
      if (j == 0)
        for (int g = 0; g < 1000; ++g) {
          r[(size_t)ci][(size_t)g] = np_interp(-px[(size_t)g], neg_conf, recall, 0.0, recall[no - 1]);
          p[(size_t)ci][(size_t)g] = np_interp(-px[(size_t)g], neg_conf, precision, 1.0, precision[no - 1]);
        }
      m_rec[0] = 0.0;
      m_pre[0] = 1.0;
      for (size_t k = 0; k < no; ++k) {
        m_rec[k + 1] = recall[k];
        m_pre[k + 1] = precision[k];
      }
      m_rec[no + 1] = 1.0;
      m_pre[no + 1] = 0.0;
      for (size_t k = no + 1; k-- > 0;) m_pre[k] = std::max(m_pre[k], m_pre[k + 1]);   // the precision envelope
      for (int g = 0; g < 101; ++g) y[(size_t)g] = np_interp(x101[(size_t)g], m_rec, m_pre, m_pre[0], m_pre[no + 1]);
      double area = 0.0;   // numpy.trapz
      for (int g = 0; g < 100; ++g) area += (x101[(size_t)g + 1] - x101[(size_t)g]) * (y[(size_t)g + 1] + y[(size_t)g]) / 2.0;
      ap[(size_t)ci][(size_t)j] = area;
    }
  }
  // f1 = 2 * p * r / (p + r + eps);  i = smooth(f1.mean(0), 0.1).argmax()
  std::vector<double> mean_f1(1000);
  for (int g = 0; g < 1000; ++g) {
    double acc = 0.0;
    for (int ci = 0; ci < nc; ++ci) {
      const double pv = p[(size_t)ci][(size_t)g], rv = r[(size_t)ci][(size_t)g];
      const double f1 = 2.0 * pv * rv / (pv + rv + eps);
      acc = ci == 0 ? f1 : acc + f1;
    }
    mean_f1[(size_t)g] = acc / (double)nc;
  }
  const int nf = 101, half = nf / 2;   // round(1000 * 0.1 * 2) // 2 + 1
  std::vector<double> yp((size_t)(1000 + 2 * half));
  for (int k = 0; k < half; ++k) {
    yp[(size_t)k] = 1.0 * mean_f1[0];
    yp[(size_t)(half + 1000 + k)] = 1.0 * mean_f1[999];
  }
  for (int g = 0; g < 1000; ++g) yp[(size_t)(half + g)] = mean_f1[(size_t)g];
  const double tap = 1.0 / (double)nf;
  int best = 0;
  double best_v = 0.0;
  for (int g = 0; g < 1000; ++g) {
    double acc = 0.0;
    for (int k = 0; k < nf; ++k) acc += yp[(size_t)(g + k)] * tap;
    if (g == 0 || acc > best_v) {
      best = g;
      best_v = acc;
    }
  }
  s->grid_index = best;
  double sp = 0.0, sr = 0.0, s50 = 0.0, sap = 0.0;
  for (int ci = 0; ci < nc; ++ci) {
    const double pv = p[(size_t)ci][(size_t)best], rv = r[(size_t)ci][(size_t)best];
    const double tpv = std::nearbyint(rv * nt[(size_t)ci]), fpv = std::nearbyint(tpv / (pv + eps) - tpv);
    double a = 0.0;
    for (int j = 0; j < n_iou; ++j) a += ap[(size_t)ci][(size_t)j];
    a /= (double)n_iou;
    sp += pv;
    sr += rv;
    s50 += ap[(size_t)ci][0];
    sap += a;
    if (ci < VP_DET_MAX_CLASSES) {
      s->ap50[ci] = ap[(size_t)ci][0];
      s->ap[ci] = a;
      s->tp[ci] = tpv;
      s->fp[ci] = fpv;
    }
  }
  s->precision = sp / (double)nc;
  s->recall = sr / (double)nc;
  s->map50 = s50 / (double)nc;
  s->map = sap / (double)nc;
}

// ---- the lane part
static_assert(sizeof(vp_metric_lanes_frame) == sizeof(vp::LanesRecord) && offsetof(vp_metric_lanes_frame, edge) == offsetof(vp::LanesRecord, edge) &&
                  offsetof(vp_metric_lanes_frame, score) == offsetof(vp::LanesRecord, score) && offsetof(vp_metric_lanes_frame, nonfinite) == offsetof(vp::LanesRecord, nonfinite) &&
                  sizeof(vp_metric_rows_line) == sizeof(vp::RowsRecord) && offsetof(vp_metric_rows_line, tp) == offsetof(vp::RowsRecord, tp) &&
                  offsetof(vp_metric_rows_line, target_valid) == offsetof(vp::RowsRecord, target_valid),
              "vp_metric_lanes_frame / vp_metric_rows_line are the records the kernels write");
static_assert(VP_LANES_GT_PLANES == vp::kLanesGtPlanes && VP_LANES_GT_BITS == vp::kLanesGtBits && VP_LANES_GT_BITS_4X == vp::kLanesGtBits4x && VP_ROWS_MAX_THR == vp::kMetricRowsMaxThr &&
                  VP_ROWS_MAX_LINES == vp::kMetricRowsMaxLines && VP_ROWS_MAX_ROWS == vp::kMetricRowsMaxRows,
              "the header's lane constants are the kernels'");

// the dataset score of train_ego_lanes.py:387-417 and its parts: means over the frames without NaN, in double
void lanes_summary(const std::vector<vp_metric_lanes_frame>& recs, vp_metric_lanes_summary* s) {
  std::memset(s, 0, sizeof(*s));
  int scored = 0;
  for (const vp_metric_lanes_frame& r : recs) {
    ++s->frames;
    if (std::isnan(r.score)) {
      ++s->nan_frames;
      continue;
    }
    ++scored;
    s->score += (double)r.score;
    for (int c = 0; c < 3; ++c) {
      s->loss[c] += (double)r.loss[c];
      s->bce[c] += (double)r.bce[c];
      double e = 0.0;
      for (int k = 0; k < 5; ++k) e += (double)r.edge[c][k];
      s->edge[c] += e / 5.0;
    }
  }
  const double nan = std::nan("");
  s->score = scored ? s->score / scored : nan;
  for (int c = 0; c < 3; ++c) {
    s->loss[c] = scored ? s->loss[c] / scored : nan;
    s->bce[c] = scored ? s->bce[c] / scored : nan;
    s->edge[c] = scored ? s->edge[c] / scored : nan;
  }
}

// compute_vector_ap (Models/training/auto_steer_util.py:353-399) in double, statement for statement; the table in the caller's order
void rows_ap(const uint32_t* tp_in, const float* conf_in, int n, const double* thr, int n_thr, vp_metric_rows_summary* s) {
  const double eps = 1e-16, nan = std::nan("");
  std::memset(s, 0, sizeof(*s));
  s->lines = n;
  s->n_thr = n_thr;
  s->map50 = nan;
  for (int j = 0; j < n_thr; ++j)
    if (thr[j] == 0.05) s->map50 = 0.0;
  if (n == 0) return;   // val(): "No valid predictions found", every score 0
  // i = numpy.argsort(-conf); equal conf keep line order, a NaN goes last
  std::vector<int> order((size_t)n);
  for (int i = 0; i < n; ++i) order[(size_t)i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
    const float ca = conf_in[a], cb = conf_in[b];
    if (std::isnan(ca)) return false;
    if (std::isnan(cb)) return true;
    return ca > cb;
  });
  const std::vector<double> x101 = np_linspace01(101);
  const size_t no = (size_t)n;
  std::vector<double> m_rec(no + 2), m_pre(no + 2), y(101);
  double sum_p = 0.0, sum_r = 0.0, sum_ap = 0.0;
  for (int j = 0; j < n_thr; ++j) {
    long long tpc = 0, fpc = 0;
    double mp = 0.0, mr = 0.0;
    for (size_t k = 0; k < no; ++k) {
      const int t = (int)((tp_in[order[k]] >> j) & 1u);
      tpc += t;
      fpc += 1 - t;
      const double precision = (double)tpc / ((double)(tpc + fpc) + eps), recall = (double)tpc / ((double)n + eps);
      m_pre[k + 1] = precision;
      m_rec[k + 1] = recall;
      mp += precision;
      mr += recall;
    }
    m_rec[0] = 0.0;
    m_pre[0] = 0.0;
    m_rec[no + 1] = 1.0;
    m_pre[no + 1] = 0.0;
    for (size_t k = no + 1; k-- > 0;) m_pre[k] = std::max(m_pre[k], m_pre[k + 1]);   // the precision envelope
    for (int g = 0; g < 101; ++g) y[(size_t)g] = np_interp(x101[(size_t)g], m_rec, m_pre, m_pre[0], m_pre[no + 1]);
    double area = 0.0;   // numpy.trapz
    for (int g = 0; g < 100; ++g) area += (x101[(size_t)g + 1] - x101[(size_t)g]) * (y[(size_t)g + 1] + y[(size_t)g]) / 2.0;
    s->ap[j] = area;
    if (thr[j] == 0.05) s->map50 = area;
    sum_ap += area;
    sum_p += mp / (double)n;
    sum_r += mr / (double)n;
  }
  s->precision = sum_p / (double)n_thr;
  s->recall = sum_r / (double)n_thr;
  s->mean_ap = sum_ap / (double)n_thr;
}

}  // namespace

extern "C" {

int vp_metric_create(vp_metric** out, int gpu_id, int max_frames, char* err, size_t err_len) {
  if (!out) return VP_ERR_ARG;
  *out = nullptr;
  try {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) throw std::runtime_error("HIP error: no HIP device visible: a vp_metric lives on the device");
    if (gpu_id < 0 || gpu_id >= n) throw std::invalid_argument("gpu_id out of range");
    auto m = std::make_unique<vp_metric>();
    m->impl = std::make_unique<vp::Metric>(gpu_id, max_frames);
    *out = m.release();
    return VP_OK;
  } catch (const std::invalid_argument& ex) {
    set_err(err, err_len, ex.what());
    return VP_ERR_ARG;
  } catch (const std::exception& ex) {
    set_err(err, err_len, ex.what());
    return VP_ERR_HIP;
  }
}

void vp_metric_destroy(vp_metric* m) { delete m; }

const char* vp_metric_last_error(const vp_metric* m) { return m ? m->err.c_str() : "null metric"; }

int vp_metric_reset(vp_metric* m) {
  return metric_guarded(m, [&](vp::Metric& g) { g.reset(); });
}

int vp_metric_add_seg(vp_metric* m, vp_engine* e, const uint8_t* gt, int gt_on_device, int gt_form) {
  return metric_guarded(m, [&](vp::Metric& g) {
    vp::Engine& en = metric_engine(e, "vp_metric_add_seg");
    if (!gt) throw std::invalid_argument("vp_metric_add_seg: null ground truth");
    g.add_seg(en, gt, gt_on_device != 0, gt_form);
  });
}

int vp_metric_add_depth(vp_metric* m, vp_engine* e, const float* gt, int gt_on_device) {
  return metric_guarded(m, [&](vp::Metric& g) {
    vp::Engine& en = metric_engine(e, "vp_metric_add_depth");
    if (!gt) throw std::invalid_argument("vp_metric_add_depth: null ground truth");
    g.add_depth(en, gt, gt_on_device != 0);
  });
}

int vp_metric_add_seg_pair(vp_metric* m, vp_engine* e, vp_engine* ref) {
  return metric_guarded(m, [&](vp::Metric& g) { g.add_seg_pair(metric_engine(e, "vp_metric_add_seg_pair"), metric_engine(ref, "vp_metric_add_seg_pair")); });
}

int vp_metric_add_depth_pair(vp_metric* m, vp_engine* e, vp_engine* ref) {
  return metric_guarded(m, [&](vp::Metric& g) { g.add_depth_pair(metric_engine(e, "vp_metric_add_depth_pair"), metric_engine(ref, "vp_metric_add_depth_pair")); });
}

int vp_metric_frames(const vp_metric* m) { return m && m->impl ? m->impl->frames() : VP_ERR_ARG; }

int vp_metric_fetch(vp_metric* m, vp_metric_frame* records, int cap, vp_metric_summary* summary) {
  return metric_guarded(m, [&](vp::Metric& g) {
    if (cap < 0 || (cap > 0 && !records)) throw std::invalid_argument("vp_metric_fetch: cap < 0, or null records with cap > 0");
    m->host.resize((size_t)g.frames());
    g.fetch(reinterpret_cast<vp::MetricRecord*>(m->host.data()), g.frames());
    const int n = std::min(cap, g.frames());
    if (n) std::memcpy(records, m->host.data(), (size_t)n * sizeof(vp_metric_frame));
    if (summary) metric_summary(m->host, summary);
  });
}

int vp_metric_add_seg_logits(vp_metric* m, const float* logits_chw, int on_device, int c, int h, int w, const uint8_t* gt, int gt_on_device, int gt_form) {
  return metric_guarded(m, [&](vp::Metric& g) { g.add_seg_logits(logits_chw, on_device != 0, c, h, w, gt, gt_on_device != 0, gt_form); });
}

int vp_metric_add_depth_plane(vp_metric* m, const float* pred, int pred_on_device, const float* gt, int gt_on_device, int h, int w) {
  return metric_guarded(m, [&](vp::Metric& g) { g.add_depth_plane(pred, pred_on_device != 0, gt, gt_on_device != 0, h, w); });
}

// ---- the detector part
int vp_metric_add_det(vp_metric* m, vp_engine* e, const float* labels, int n_labels, float conf, float iou, const float* iou_v, int n_iou) {
  return metric_guarded(m, [&](vp::Metric& g) { g.add_det(metric_engine(e, "vp_metric_add_det"), labels, n_labels, conf, iou, iou_v, n_iou); });
}

int vp_metric_add_det_pair(vp_metric* m, vp_engine* e, vp_engine* ref, float label_conf, float conf, float iou, const float* iou_v, int n_iou) {
  return metric_guarded(m, [&](vp::Metric& g) {
    g.add_det_pair(metric_engine(e, "vp_metric_add_det_pair"), metric_engine(ref, "vp_metric_add_det_pair"), label_conf, conf, iou, iou_v, n_iou);
  });
}

int vp_metric_add_det_raw(vp_metric* m, const float* raw, int on_device, int nc, int nb, int net_h, int net_w, const float* labels, int n_labels, float conf, float iou,
                          const float* iou_v, int n_iou) {
  return metric_guarded(m, [&](vp::Metric& g) { g.add_det_raw(raw, on_device != 0, nc, nb, net_h, net_w, labels, n_labels, conf, iou, iou_v, n_iou); });
}

int vp_metric_det_frames(const vp_metric* m) { return m && m->impl ? m->impl->det_frames() : VP_ERR_ARG; }

int vp_metric_fetch_det(vp_metric* m, vp_metric_det_frame* frames_out, int frames_cap, vp_metric_det_row* rows_out, int rows_cap, vp_metric_det_summary* summary) {
  return metric_guarded(m, [&](vp::Metric& g) {
    if (frames_cap < 0 || rows_cap < 0 || (frames_cap > 0 && !frames_out) || (rows_cap > 0 && !rows_out))
      throw std::invalid_argument("vp_metric_fetch_det: a negative capacity, or a null buffer with a capacity above 0");
    g.fetch_det(&m->det_frames, &m->det_rows, &m->det_label_cls);
    const size_t nf = std::min((size_t)frames_cap, m->det_frames.size()), nr = std::min((size_t)rows_cap, m->det_rows.size());
    if (nf) std::memcpy(frames_out, m->det_frames.data(), nf * sizeof(vp_metric_det_frame));
    if (nr) std::memcpy(rows_out, m->det_rows.data(), nr * sizeof(vp_metric_det_row));
    if (summary) {
      const size_t n = m->det_rows.size();
      std::vector<uint32_t> tp(n);
      std::vector<float> conf(n), cls(n);
      for (size_t i = 0; i < n; ++i) {
        tp[i] = m->det_rows[i].tp;
        conf[i] = m->det_rows[i].conf;
        cls[i] = m->det_rows[i].cls;
      }
      summary->frames = (int)m->det_frames.size();
      det_ap(tp.data(), conf.data(), cls.data(), (int)n, m->det_label_cls.data(), (int)m->det_label_cls.size(), std::max(1, g.det_n_iou()), summary);
    }
  });
}

int vp_metric_det_ap(const uint32_t* tp, const float* conf, const float* det_cls, int n_rows, const float* label_cls, int n_labels, int n_iou, vp_metric_det_summary* summary) {
  if (!summary || n_rows < 0 || n_labels < 0 || n_iou < 1 || n_iou > VP_DET_MAX_IOU || (n_rows > 0 && (!tp || !conf || !det_cls)) || (n_labels > 0 && !label_cls)) return VP_ERR_ARG;
  try {
    summary->frames = 0;
    det_ap(tp, conf, det_cls, n_rows, label_cls, n_labels, n_iou, summary);
    return VP_OK;
  } catch (const std::exception&) {
    return VP_ERR_STATE;
  }
}

// ---- the lane part
int vp_metric_add_lanes(vp_metric* m, vp_engine* e, const void* gt, int gt_on_device, int gt_form) {
  return metric_guarded(m, [&](vp::Metric& g) {
    vp::Engine& en = metric_engine(e, "vp_metric_add_lanes");
    if (!gt) throw std::invalid_argument("vp_metric_add_lanes: null ground truth");
    g.add_lanes(en, gt, gt_on_device != 0, gt_form);
  });
}

int vp_metric_add_lanes_pair(vp_metric* m, vp_engine* e, vp_engine* ref) {
  return metric_guarded(m, [&](vp::Metric& g) { g.add_lanes_pair(metric_engine(e, "vp_metric_add_lanes_pair"), metric_engine(ref, "vp_metric_add_lanes_pair")); });
}

int vp_metric_add_lanes_logits(vp_metric* m, const float* logits_chw, int on_device, int h, int w, const void* gt, int gt_on_device, int gt_form) {
  return metric_guarded(m, [&](vp::Metric& g) { g.add_lanes_logits(logits_chw, on_device != 0, h, w, gt, gt_on_device != 0, gt_form); });
}

int vp_metric_lanes_frames(const vp_metric* m) { return m && m->impl ? m->impl->lanes_frames() : VP_ERR_ARG; }

int vp_metric_fetch_lanes(vp_metric* m, vp_metric_lanes_frame* records, int cap, vp_metric_lanes_summary* summary) {
  return metric_guarded(m, [&](vp::Metric& g) {
    if (cap < 0 || (cap > 0 && !records)) throw std::invalid_argument("vp_metric_fetch_lanes: cap < 0, or null records with cap > 0");
    std::vector<vp_metric_lanes_frame> host((size_t)g.lanes_frames());
    g.fetch_lanes(reinterpret_cast<vp::LanesRecord*>(host.data()), g.lanes_frames());
    const int n = std::min(cap, g.lanes_frames());
    if (n) std::memcpy(records, host.data(), (size_t)n * sizeof(vp_metric_lanes_frame));
    if (summary) lanes_summary(host, summary);
  });
}

int vp_metric_add_rows(vp_metric* m, vp_engine* e, const float* target_xp, const float* target_h, const double* thr, int n_thr) {
  return metric_guarded(m, [&](vp::Metric& g) { g.add_rows(metric_engine(e, "vp_metric_add_rows"), target_xp, target_h, thr, n_thr); });
}

int vp_metric_add_rows_pair(vp_metric* m, vp_engine* e, vp_engine* ref, const double* thr, int n_thr) {
  return metric_guarded(m, [&](vp::Metric& g) { g.add_rows_pair(metric_engine(e, "vp_metric_add_rows_pair"), metric_engine(ref, "vp_metric_add_rows_pair"), thr, n_thr); });
}

int vp_metric_add_rows_raw(vp_metric* m, const float* xp, const float* h_vector, const float* target_xp, const float* target_h, int n_lines, int rows, const double* thr,
                           int n_thr) {
  return metric_guarded(m, [&](vp::Metric& g) { g.add_rows_raw(xp, h_vector, target_xp, target_h, n_lines, rows, thr, n_thr); });
}

int vp_metric_rows_lines(const vp_metric* m) { return m && m->impl ? m->impl->rows_lines() : VP_ERR_ARG; }

int vp_metric_fetch_rows(vp_metric* m, vp_metric_rows_line* records, int cap, vp_metric_rows_summary* summary) {
  return metric_guarded(m, [&](vp::Metric& g) {
    if (cap < 0 || (cap > 0 && !records)) throw std::invalid_argument("vp_metric_fetch_rows: cap < 0, or null records with cap > 0");
    std::vector<vp_metric_rows_line> host((size_t)g.rows_lines());
    g.fetch_rows(reinterpret_cast<vp::RowsRecord*>(host.data()), g.rows_lines());
    const int n = std::min(cap, g.rows_lines());
    if (n) std::memcpy(records, host.data(), (size_t)n * sizeof(vp_metric_rows_line));
    if (summary) {
      std::vector<uint32_t> tp(host.size());
      std::vector<float> conf(host.size());
      for (size_t i = 0; i < host.size(); ++i) {
        tp[i] = host[i].tp;
        conf[i] = host[i].conf;
      }
      rows_ap(tp.data(), conf.data(), (int)host.size(), g.rows_thr(), g.rows_n_thr(), summary);
    }
  });
}

int vp_metric_rows_ap(const uint32_t* tp, const float* conf, int n_lines, const double* thr, int n_thr, vp_metric_rows_summary* summary) {
  if (!summary || n_lines < 0 || !thr || n_thr < 1 || n_thr > VP_ROWS_MAX_THR || (n_lines > 0 && (!tp || !conf))) return VP_ERR_ARG;
  for (int k = 0; k < n_thr; ++k)
    if (thr[k] != thr[k]) return VP_ERR_ARG;
  try {
    rows_ap(tp, conf, n_lines, thr, n_thr, summary);
    return VP_OK;
  } catch (const std::exception&) {
    return VP_ERR_STATE;
  }
}

// ---- the label part
static_assert(sizeof(vp_label_frame) == sizeof(vp::LabelRecord) && offsetof(vp_label_frame, freq) == offsetof(vp::LabelRecord, freq) &&
                  offsetof(vp_label_frame, nonfinite) == offsetof(vp::LabelRecord, nonfinite) && offsetof(vp_label_frame, min) == offsetof(vp::LabelRecord, mn) &&
                  offsetof(vp_label_frame, max) == offsetof(vp::LabelRecord, mx) && VP_LABEL_F32 == vp::kLabelF32 && VP_LABEL_F64 == vp::kLabelF64,
              "vp_label_frame is the record the kernels write");

int vp_metric_add_seg_label(vp_metric* m, vp_engine* e, const uint8_t* label, int channels, int h, int w, int stride_bytes, const int* crop_ltrb, const uint8_t* colours,
                            int n_colours) {
  return metric_guarded(m, [&](vp::Metric& g) { g.add_seg_label(metric_engine(e, "vp_metric_add_seg_label"), label, channels, h, w, stride_bytes, crop_ltrb, colours, n_colours); });
}

int vp_metric_add_depth_label(vp_metric* m, vp_engine* e, const void* label, int dtype, int h, int w, int stride_elems) {
  return metric_guarded(m, [&](vp::Metric& g) { g.add_depth_label(metric_engine(e, "vp_metric_add_depth_label"), label, dtype, h, w, stride_elems); });
}

int vp_metric_add_seg_logits_label(vp_metric* m, const float* logits_chw, int on_device, int c, int oh, int ow, const uint8_t* label, int channels, int h, int w,
                                   int stride_bytes, const int* crop_ltrb, const uint8_t* colours, int n_colours) {
  return metric_guarded(m, [&](vp::Metric& g) { g.add_seg_logits_label(logits_chw, on_device != 0, c, oh, ow, label, channels, h, w, stride_bytes, crop_ltrb, colours, n_colours); });
}

int vp_metric_add_depth_plane_label(vp_metric* m, const float* pred, int pred_on_device, int oh, int ow, const void* label, int dtype, int h, int w, int stride_elems) {
  return metric_guarded(m, [&](vp::Metric& g) { g.add_depth_plane_label(pred, pred_on_device != 0, oh, ow, label, dtype, h, w, stride_elems); });
}

int vp_metric_label_frames(const vp_metric* m) { return m && m->impl ? m->impl->label_frames() : VP_ERR_ARG; }

int vp_metric_fetch_labels(vp_metric* m, vp_label_frame* records, int cap) {
  return metric_guarded(m, [&](vp::Metric& g) {
    if (cap < 0 || (cap > 0 && !records)) throw std::invalid_argument("vp_metric_fetch_labels: cap < 0, or null records with cap > 0");
    const int n = std::min(cap, g.label_frames());
    g.fetch_labels(reinterpret_cast<vp::LabelRecord*>(records), n);
  });
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------- vp_lanes
namespace {

static_assert(VP_LANES_MAX_WINDOWS == 2 * vp::kLaneMaxSteps && VP_LANES_MAX_POINTS == 2 * vp::kLaneRunPoints && VP_LANES_SINGULAR == vp::kLanesSingular &&
                  VP_LANES_SMOOTHED == vp::kLanesSmoothed && sizeof(long long) == sizeof(int64_t),
              "vp_lanes_result holds what the kernel's record and the host fit hold");

template <class F>
int lanes_guarded(vp_lanes* l, F&& fn) {
  if (!l || !l->impl) return VP_ERR_ARG;
  try {
    fn(*l->impl);
    return VP_OK;
  } catch (const std::invalid_argument& ex) {
    l->err = ex.what();
    return VP_ERR_ARG;
  } catch (const std::exception& ex) {
    l->err = ex.what();
    return std::strncmp(ex.what(), "HIP error", 9) == 0 ? VP_ERR_HIP : VP_ERR_STATE;
  }
}

void lanes_result_lane(const vp::LaneFilterLane& r, const vp::LanesFit& f, vp_lanes_lane* o) {
  std::memset(o, 0, sizeof(*o));
  o->start_x = r.start_x, o->start_y = r.start_y;
  o->n_windows_up = r.n_windows[0], o->n_windows_down = r.n_windows[1];
  o->n_points_up = r.n_points[0], o->n_points_down = r.n_points[1];
  o->min_y = r.min_y, o->max_y = r.max_y;
  for (int k = 0; k < 5; ++k) o->S[k] = r.S[k];
  for (int k = 0; k < 3; ++k) o->T[k] = r.T[k];
  int at = 0;
  for (int run = 0; run < 2; ++run)
    for (int i = 0; i < r.n_windows[run] && i < vp::kLaneMaxSteps; ++i, ++at)
      for (int k = 0; k < 4; ++k) o->windows[at][k] = r.win[run][i][k];
  o->order = f.order, o->flags = f.flags, o->coeffs_valid = f.coeffs_valid;
  for (int k = 0; k < 6; ++k) o->raw_coeffs[k] = f.raw[k], o->coeffs[k] = f.coeffs[k];
}

}  // namespace

extern "C" {

int vp_lanes_create(vp_lanes** out, int gpu_id, int capacity, char* err, size_t err_len) {
  if (!out) return VP_ERR_ARG;
  *out = nullptr;
  try {
    if (capacity < 1 || capacity > 4096) throw std::invalid_argument("vp_lanes_create: capacity " + std::to_string(capacity) + " (1 .. 4096)");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) throw std::runtime_error("HIP error: no HIP device visible: a vp_lanes lives on the device");
    if (gpu_id < 0 || gpu_id >= n) throw std::invalid_argument("gpu_id out of range");
    auto l = std::make_unique<vp_lanes>();
    l->impl = std::make_unique<vp::Lanes>(gpu_id, capacity);
    *out = l.release();
    return VP_OK;
  } catch (const std::invalid_argument& ex) {
    set_err(err, err_len, ex.what());
    return VP_ERR_ARG;
  } catch (const std::exception& ex) {
    set_err(err, err_len, ex.what());
    return VP_ERR_HIP;
  }
}

void vp_lanes_destroy(vp_lanes* l) { delete l; }

const char* vp_lanes_last_error(const vp_lanes* l) { return l ? l->err.c_str() : "null lane filter"; }

int vp_lanes_set_smoothing(vp_lanes* l, float smoothing) {
  return lanes_guarded(l, [&](vp::Lanes& g) {
    if (!(smoothing >= 0.0f && smoothing <= 1.0f)) throw std::invalid_argument("vp_lanes_set_smoothing: a factor outside 0 .. 1");
    g.set_smoothing(smoothing);
  });
}

int vp_lanes_reset(vp_lanes* l) {
  return lanes_guarded(l, [&](vp::Lanes& g) { g.reset(); });
}

int vp_lanes_add(vp_lanes* l, vp_engine* e, float threshold) {
  return lanes_guarded(l, [&](vp::Lanes& g) { g.add(metric_engine(e, "vp_lanes_add"), threshold); });
}

int vp_lanes_add_logits(vp_lanes* l, const float* logits_3x80x160, float threshold) {
  return lanes_guarded(l, [&](vp::Lanes& g) { g.add_logits(logits_3x80x160, threshold); });
}

int vp_lanes_pending(const vp_lanes* l) { return l && l->impl ? l->impl->pending() : VP_ERR_ARG; }

int vp_lanes_fetch(vp_lanes* l, vp_lanes_result* out, int max, int* n) {
  return lanes_guarded(l, [&](vp::Lanes& g) {
    if (!n || max < 0 || (max > 0 && !out)) throw std::invalid_argument("vp_lanes_fetch: null n, max < 0, or null out with max > 0");
    const int count = std::min(max, g.pending());
    l->recs.resize((size_t)count);
    l->fits.resize(2 * (size_t)count);
    g.fetch(l->recs.data(), l->fits.data(), count);
    for (int i = 0; i < count; ++i)
      for (int k = 0; k < 2; ++k) lanes_result_lane(l->recs[i].lane[k], l->fits[2 * i + k], &out[i].lane[k]);
    *n = count;
  });
}

int vp_lanes_fetch_points(vp_lanes* l, int record_index, int lane, uint8_t* xy, int max_points, int* n) {
  return lanes_guarded(l, [&](vp::Lanes& g) {
    if (!n) throw std::invalid_argument("vp_lanes_fetch_points: null n");
    *n = g.fetch_points(record_index, lane, xy, max_points);
  });
}

int vp_lanes_fit(const int64_t S[5], const int64_t T[3], int order, double out[3], int* singular) {
  try {
    if (!S || !T || !out) return VP_ERR_ARG;
    long long s[5], t[3];
    for (int k = 0; k < 5; ++k) s[k] = S[k];
    for (int k = 0; k < 3; ++k) t[k] = T[k];
    const bool ok = vp::lanes_fit(s, t, order, out);
    if (singular) *singular = ok ? 0 : 1;
    return VP_OK;
  } catch (const std::exception&) {
    return VP_ERR_ARG;
  }
}

}  // extern "C"
namespace {
// (hi, lo) planes of an activation, NHWC with padded channels on the device -> fp16 bit patterns [Creal][H][W] on the host
void read_planes_chw(vp::Engine& g, const vp::Act* a, uint16_t* out_hi, uint16_t* out_lo) {
  std::vector<uint16_t> buf(a->elems());
  for (int plane = 0; plane < 2; ++plane) {
    uint16_t* dst = plane ? out_lo : out_hi;
    const vp::half_t* src = plane ? a->lo : a->hi;
    if (!dst) continue;
    if (!src) {
      std::memset(dst, 0, (size_t)a->Creal * a->H * a->W * sizeof(uint16_t));
      continue;
    }
    g.copy_d2h(buf.data(), src, buf.size() * sizeof(uint16_t));
    for (int c = 0; c < a->Creal; ++c)
      for (int i = 0; i < a->H * a->W; ++i) dst[(size_t)c * a->H * a->W + i] = buf[(size_t)i * a->C + c];
  }
}
// on_range: what a vp::RangeError (a weight beyond the fp16 range) becomes -- VP_ERR_RANGE for vp_op_upconv alone
template <class F>
int op_guarded(char* err, size_t err_len, F&& f, int on_range = VP_ERR_HIP) {
  try {
    f();
    return VP_OK;
  } catch (const std::invalid_argument& ex) {
    set_err(err, err_len, ex.what());
    return VP_ERR_ARG;
  } catch (const vp::RangeError& ex) {
    set_err(err, err_len, ex.what());
    return on_range;
  } catch (const std::exception& ex) {
    set_err(err, err_len, ex.what());
    return VP_ERR_HIP;
  }
}
// VP_ACT_SCALE operator entries: the planes hold x * 2^-s -- the host scales the TRUE-valued argument (exact) before it is split; e = 0: the argument itself
void upload_act_scaled(vp::Engine& g, vp::Act* a, const float* chw, int e) {
  if (e == 0) return g.upload_act(a, chw);
  if (e < -60 || e > 60) throw std::invalid_argument("exponent out of range (-60 .. 60)");
  std::vector<float> v(chw, chw + (size_t)a->Creal * a->H * a->W);
  for (float& x : v) x = std::ldexp(x, -e);
  g.upload_act(a, v.data());
}
// fp32 CHW values of a tensor the entry holds (Engine::read_act goes by the index in acts())
void read_act_chw(vp::Engine& g, const vp::Act* a, float* out) {
  for (size_t i = 0; i < g.acts().size(); ++i)
    if (g.acts()[i].get() == a) return g.read_act((int)i, out);
  throw std::runtime_error("read_act_chw: not a tensor of this engine");
}
float* to_device(vp::Engine& g, const std::vector<float>& v) {
  float* d = g.alloc_f32(v.size());
  g.copy_h2d(d, v.data(), v.size() * sizeof(float));
  return d;
}
// vp_op_absmax / vp_op_exp_hist: fp16 bit patterns [h][w][c_pitch], lo may be null -- the refusals both share (ahead of the engine, so that they do
// not need a device), and the planes on the engine's device
void check_planes(bool pointers, int c, int h, int w, int c_pitch) {   // pointers: hi and the entry's result pointers are all there
  if (!pointers || c < 1 || h < 1 || w < 1 || c_pitch < ((c + 7) & ~7) || (c_pitch & 7) || (long long)h * w * c_pitch > (1ll << 28))
    throw std::invalid_argument("bad argument (c_pitch: a multiple of 8, at least c rounded up to 8)");
}
struct DevPlanes {
  vp::half_t *hi, *lo;
};
DevPlanes upload_planes(vp::Engine& g, const uint16_t* hi, const uint16_t* lo, size_t n) {
  DevPlanes d;
  d.hi = reinterpret_cast<vp::half_t*>(g.alloc_f32((n + 1) / 2));
  d.lo = lo ? reinterpret_cast<vp::half_t*>(g.alloc_f32((n + 1) / 2)) : nullptr;
  g.copy_h2d(d.hi, hi, n * sizeof(uint16_t));
  if (lo) g.copy_h2d(d.lo, lo, n * sizeof(uint16_t));
  return d;
}

// exps: null = the unflagged launch (vp_op_detect_head_decode); else [3][2] exponents of (box, cls) per level
void op_detect_head_decode(int gpu_id, int precision, const float* box, const float* cls, int nc, int h0, int w0, const int* exps, float* out) {
  if (!box || !cls || !out || nc < 1 || nc > 4092 || h0 < 4 || w0 < 4 || (h0 & 3) || (w0 & 3) || (long long)h0 * w0 > (1 << 22)) throw std::invalid_argument("bad argument");
  vp::Engine g(-1, nullptr, precision, gpu_id);
  vp::DetectHeadParams p{};
  size_t off = 0;
  int first = 0;
  for (int l = 0; l < 3; ++l) {
    const int h = h0 >> l, w = w0 >> l;
    vp::Act* b = g.new_act("box", 64, h, w);
    vp::Act* c = g.new_act("cls", nc, h, w);
    const int eb = exps ? exps[2 * l] : 0, ec = exps ? exps[2 * l + 1] : 0;
    upload_act_scaled(g, b, box + off * 64, eb);
    upload_act_scaled(g, c, cls + off * nc, ec);
    p.scaled |= (eb | ec) != 0;   // all 0: the unflagged parameter block
    p.lv[l].box_mul = std::ldexp(1.0f, eb);
    p.lv[l].cls_mul = std::ldexp(1.0f, ec);
    p.lv[l].box = b->view();
    p.lv[l].cls = c->view();
    p.lv[l].first = first;
    p.lv[l].stride = (float)(8 << l);
    off += (size_t)h * w;
    first += h * w;
  }
  p.nc = nc;
  p.total = first;
  p.out = g.alloc_f32((size_t)(4 + nc) * first);
  VP_HIP_CHECK(vp::launch_detect_head_decode(p, g.stream()));
  g.copy_d2h(out, p.out, (size_t)(4 + nc) * first * sizeof(float));
}

// the AutoSteer head's two kernels; exponents 0: the unflagged launches (vp_op_rowpair_conv / vp_op_lane_rows_head)
void op_rowpair_conv(int gpu_id, int precision, const float* in, int cin, int h, int w, const float* weight, const float* bias, int replicate,
                     int dst_c, int dst_off, const float* dst_init, int in_exp, int out_exp, uint16_t* out_hi, uint16_t* out_lo) {
  if (!in || !weight || !bias || !out_hi || cin < 8 || cin > 64 || (cin & 7) || h < 2 || w < 1 || (long long)h * w > (1 << 20) || dst_c < 32 || (dst_c & 31) || dst_off < 0 ||
      (dst_off & 31) || dst_off + 32 > dst_c)
    throw std::invalid_argument("bad argument (cin: a multiple of 8 up to 64; dst_c, dst_off: multiples of 32 with dst_off + 32 <= dst_c)");
  vp::Engine g(-1, nullptr, precision, gpu_id);
  const int f = replicate ? 2 : 1, ho = (h / 2) * f, wo = w * f;
  vp::Act* ti = g.new_act("in", cin, h, w);
  vp::Act* to = g.new_act("out", dst_c, ho, wo);
  upload_act_scaled(g, ti, in, in_exp);
  if (dst_init) upload_act_scaled(g, to, dst_init, out_exp);   // the whole destination carries one exponent (an alias slice shares its tensor's)
  std::vector<float> wk((size_t)2 * cin * 32);
  for (int co = 0; co < 32; ++co)
    for (int ci = 0; ci < cin; ++ci)
      for (int ky = 0; ky < 2; ++ky) wk[((size_t)ky * cin + ci) * 32 + co] = weight[((size_t)co * cin + ci) * 2 + ky];
  float* dw = to_device(g, wk);
  float* db = g.alloc_f32(32);
  g.copy_h2d(db, bias, 32 * sizeof(float));
  vp::RowpairConvParams q{};
  q.in = ti->view();
  q.cin = cin;
  q.w = dw;
  q.b = db;
  q.out = to->view();
  q.out.hi += dst_off;   // the alias-slice convention: pixel * Cstore + channel
  if (q.out.lo) q.out.lo += dst_off;
  q.replicate = replicate ? 1 : 0;
  q.scaled = (in_exp | out_exp) != 0;   // both 0: the unflagged parameter block
  q.in_mul = std::ldexp(1.0f, in_exp);
  q.out_mul = std::ldexp(1.0f, -out_exp);
  VP_HIP_CHECK(vp::launch_rowpair_conv(q, g.stream()));
  read_planes_chw(g, to, out_hi, out_lo);
}

void op_lane_rows_head(int gpu_id, int precision, const float* features, int cin, int h, int w, const float* c1_w, float c1_b, const float* c2_w,
                       float c2_b, const float* h1_w, float h1_b, const float* h2_w, float h2_b, int in_exp, float* out_2xh) {
  if (!features || !c1_w || !c2_w || !h1_w || !h2_w || !out_2xh || cin < 8 || cin > 64 || (cin & 7) || h < 1 || h > 4096 || w != 256)
    throw std::invalid_argument("bad argument (cin: a multiple of 8 up to 64; w = 256)");
  vp::Engine g(-1, nullptr, precision, gpu_id);
  vp::Act* tf = g.new_act("features", cin, h, w);
  upload_act_scaled(g, tf, features, in_exp);
  std::vector<float> wk((size_t)9 * cin * 2), hk(36);
  for (int t = 0; t < 9; ++t)
    for (int ci = 0; ci < cin; ++ci) {
      wk[((size_t)t * cin + ci) * 2 + 0] = c1_w[(size_t)ci * 9 + t];
      wk[((size_t)t * cin + ci) * 2 + 1] = c2_w[(size_t)ci * 9 + t];
    }
  for (int i = 0; i < 16; ++i) {
    hk[i] = h1_w[i];
    hk[16 + i] = h2_w[i];
  }
  hk[32] = c1_b;
  hk[33] = c2_b;
  hk[34] = h1_b;
  hk[35] = h2_b;
  float* dw = to_device(g, wk);
  float* dh = to_device(g, hk);
  vp::LaneRowsHeadParams q{};
  q.features = tf->view();
  q.cin = cin;
  q.w = dw;
  q.hw = dh;
  q.out = g.alloc_f32((size_t)2 * h);
  q.scaled = in_exp != 0;   // 0: the unflagged parameter block
  q.in_mul = std::ldexp(1.0f, in_exp);
  VP_HIP_CHECK(vp::launch_lane_rows_head(q, g.stream()));
  g.copy_d2h(out_2xh, q.out, (size_t)2 * h * sizeof(float));
}
}  // namespace
extern "C" {

int vp_op_conv2d(int gpu_id, int precision, int mode, const float* in, int cin, int h, int w, const float* weight, const float* bias,
                 int cout, int ks, int act, int res_mode, const float* res, int tile, int bk, int nsplit, float* out, char* err,
                 size_t err_len) {
  return op_guarded(err, err_len, [&] {
    if (!in || !weight || !bias || !out || cin < 1 || cout < 1 || h < 1 || w < 1) throw std::invalid_argument("bad argument");
    vp::Engine g(-1, nullptr, precision, gpu_id);
    vp::Act* a = g.new_act("in", cin, h, w);
    g.upload_act(a, in);
    const int oh = mode >= 1 ? 2 * h : h, ow = mode >= 1 ? 2 * w : w;
    if (mode == 2) {  // ConvTranspose2d(k2, s2)(in) + Conv2d 1x1(skip): `res` is the skip INPUT [res_mode channels][2h][2w]
      const int cs = res_mode;
      if (!res || cs < 1) throw std::invalid_argument("mode 2: res = skip tensor, res_mode = its channel count");
      vp::Act* sk = g.new_act("skip", cs, oh, ow);
      g.upload_act(sk, res);
      const size_t wt_n = (size_t)cin * cout * 4;
      std::vector<float> wt(weight, weight + wt_n), ws(weight + wt_n, weight + wt_n + (size_t)cout * cs), bt(bias, bias + cout),
          bs(bias + cout, bias + 2 * cout);
      vp::Act* y = g.add_convT_skip("op", "op.skip", a, sk, wt, bt, ws, bs, cout);
      g.run_eager();
      g.sync();
      return read_act_chw(g, y, out);
    }
    if (mode == 3) {  // a head's logits convolution: 3x3, fp32 NCHW output straight from the kernel (STORE_NCHW_F32)
      if (ks != 3 || act != 0 || res_mode != 0) throw std::invalid_argument("mode 3: 3x3, no activation, no residual");
      float* d_out = g.alloc_f32((size_t)cout * h * w);
      vp::ConvOpts lo;
      lo.tile = tile;
      lo.logits_out = d_out;
      const size_t wn3 = (size_t)cin * cout * 9;
      g.add_conv("op", a, std::vector<float>(weight, weight + wn3), std::vector<float>(bias, bias + cout), cout, 3, lo);
      g.run_eager();
      g.sync();
      return g.copy_d2h(out, d_out, (size_t)cout * h * w * sizeof(float));
    }
    vp::ConvOpts o;
    o.act = act;
    o.tile = tile;
    o.bk = bk;
    o.nsplit = nsplit;
    vp::Act* r = nullptr;
    if (res_mode != 0) {
      if (!res) throw std::invalid_argument("res_mode set but res is null");
      r = g.new_act("res", cout, oh, ow);
      g.upload_act(r, res);
      o.res_mode = res_mode;
      o.res = r;
    }
    const size_t wn = (size_t)cin * cout * (mode == 1 ? 4 : ks * ks);
    std::vector<float> wv(weight, weight + wn), bv(bias, bias + cout);
    vp::Act* y = mode == 1 ? g.add_convT("op", a, wv, bv, cout, o) : g.add_conv("op", a, wv, bv, cout, ks, o);
    g.run_eager();
    g.sync();
    read_act_chw(g, y, out);
  });
}

int vp_op_detect_head_decode(int gpu_id, int precision, const float* box, const float* cls, int nc, int h0, int w0, float* out, char* err, size_t err_len) {
  return op_guarded(err, err_len, [&] { op_detect_head_decode(gpu_id, precision, box, cls, nc, h0, w0, nullptr, out); });
}

int vp_op_upsample2_cat(int gpu_id, int precision, const float* a, int ca, const float* b, int cb, int h, int w, uint16_t* out_hi, uint16_t* out_lo,
                        char* err, size_t err_len) {
  return op_guarded(err, err_len, [&] {
    if (!a || !b || !out_hi || ca < 1 || cb < 1 || h < 1 || w < 1 || (ca & 31) || (long long)h * w > (1 << 20)) throw std::invalid_argument("bad argument (ca: a multiple of 32)");
    vp::Engine g(-1, nullptr, precision, gpu_id);
    vp::Act* ta = g.new_act("a", ca, h, w);
    vp::Act* tb = g.new_act("b", cb, 2 * h, 2 * w);
    vp::Act* to = g.new_act("out", ca + cb, 2 * h, 2 * w);
    g.upload_act(ta, a);
    g.upload_act(tb, b);
    vp::Upsample2CatParams q{};
    q.a = ta->view();
    q.b = tb->view();
    q.out = to->view();
    q.a_nch = ca;
    q.b_nch = tb->C;   // padded width: the pad channels are zero and land in the output's padding
    if (ca + tb->C > to->C) q.b_nch = to->C - ca;
    VP_HIP_CHECK(vp::launch_upsample2_cat(q, g.stream()));
    read_planes_chw(g, to, out_hi, out_lo);
  });
}

int vp_op_dwconv3x3(int gpu_id, int precision, const float* in, int c, int h, int w, const float* weight, const float* bias, int act, const float* add,
                    uint16_t* out_hi, uint16_t* out_lo, char* err, size_t err_len) {
  return op_guarded(err, err_len, [&] {
    if (!in || !weight || !bias || !out_hi || c < 1 || h < 1 || w < 1 || (long long)h * w > (1 << 20)) throw std::invalid_argument("bad argument");
    vp::Engine g(-1, nullptr, precision, gpu_id);
    vp::Act* ti = g.new_act("in", c, h, w);
    vp::Act* to = g.new_act("out", c, h, w);
    g.upload_act(ti, in);
    std::vector<float> wk((size_t)9 * ti->C, 0.0f), bk(ti->C, 0.0f);
    for (int ch = 0; ch < c; ++ch) {
      for (int k = 0; k < 9; ++k) wk[(size_t)k * ti->C + ch] = weight[(size_t)ch * 9 + k];
      bk[ch] = bias[ch];
    }
    float* dw = to_device(g, wk);
    float* db = to_device(g, bk);
    vp::DwPlainParams dp{};
    dp.in = ti->view();
    dp.out = to->view();
    dp.w = dw;
    dp.b = db;
    dp.act = act;
    if (add) {
      vp::Act* tadd = g.new_act("add", c, h, w);
      g.upload_act(tadd, add);
      dp.add = tadd->view();
    }
    VP_HIP_CHECK(vp::launch_dwconv_plain(dp, g.stream()));
    read_planes_chw(g, to, out_hi, out_lo);
  });
}

// ---- the e4m3 MFMA layer (VP_MFMA_FP8): the engine's packer and launch on any map size (the dispatch rule's size floor is the engine's, not the kernel's)
int vp_op_conv3x3_f8(int gpu_id, const float* in, int cin, int h, int w, const float* weight, const float* bias, int cout, int act, int qexp,
                     uint16_t* out_f16, char* err, size_t err_len) {
  return op_guarded(err, err_len, [&] {
    if (!in || !weight || !bias || !out_f16 || cin < 1 || cout < 1 || h < 1 || w < 1 || (long long)h * w > (1 << 22)) throw std::invalid_argument("bad argument");
    if (act != 0 && act != 1) throw std::invalid_argument("vp_op_conv3x3_f8: act 0 (none) or 1 (GELU)");
    if (h < 8 || w < 16) throw std::invalid_argument("vp_op_conv3x3_f8: maps of at least 8 x 16 pixels");
    vp::Engine g(-1, nullptr, VP_FP16 | VP_MFMA_FP8, gpu_id);
    vp::Act* a = g.new_act("in", cin, h, w);
    g.upload_act(a, in);   // one fp16 plane: the values rounded to fp16
    vp::ConvOpts o;
    o.act = act;
    o.tile = 113;
    const size_t wn = (size_t)cin * cout * 9;
    vp::Act* y = g.add_conv("op", a, std::vector<float>(weight, weight + wn), std::vector<float>(bias, bias + cout), cout, 3, o);
    g.set_fp8_exps(&qexp, 1);
    g.run_eager();
    g.sync();
    read_planes_chw(g, y, out_f16, nullptr);
  });
}

int vp_op_fp8_quantize(int gpu_id, const uint16_t* f16, size_t n, int qexp, uint8_t* codes, char* err, size_t err_len) {
  return op_guarded(err, err_len, [&] {
    if (!f16 || !codes || n < 1 || n > (1u << 28) || qexp < -24 || qexp > 24) throw std::invalid_argument("bad argument (qexp: -24 .. 24)");
    vp::Engine g(-1, nullptr, VP_FP16, gpu_id);
    const DevPlanes d = upload_planes(g, f16, nullptr, n);
    uint8_t* dc = reinterpret_cast<uint8_t*>(g.alloc_f32((n + 3) / 4));
    VP_HIP_CHECK(vp::launch_fp8_quantize(d.hi, n, std::ldexp(1.0f, -qexp), dc, g.stream()));
    g.copy_d2h(codes, dc, n);
  });
}

// ---- single-operator entries of the VP_ACT_SCALE mechanism (unit tests)
int vp_op_absmax(int gpu_id, const uint16_t* hi, const uint16_t* lo, int c, int h, int w, int c_pitch, float* absmax, unsigned* nonfinite, char* err, size_t err_len) {
  return op_guarded(err, err_len, [&] {
    check_planes(hi && absmax && nonfinite, c, h, w, c_pitch);
    vp::Engine g(-1, nullptr, VP_FP16X3, gpu_id);
    const DevPlanes d = upload_planes(g, hi, lo, (size_t)h * w * c_pitch);
    unsigned* dr = reinterpret_cast<unsigned*>(g.alloc_f32(2));   // zeroed
    VP_HIP_CHECK(vp::launch_act_absmax(d.hi, d.lo, c, h, w, c_pitch, dr, g.stream()));
    unsigned r[2];
    g.copy_d2h(r, dr, sizeof(r));
    std::memcpy(absmax, &r[0], sizeof(float));
    *nonfinite = r[1];
  });
}

int vp_op_exp_hist(int gpu_id, const uint16_t* hi, const uint16_t* lo, int c, int h, int w, int c_pitch, unsigned long long* bins, unsigned long long* zeros,
                   unsigned long long* count, char* err, size_t err_len) {
  return op_guarded(err, err_len, [&] {
    check_planes(hi && bins && zeros && count, c, h, w, c_pitch);
    vp::Engine g(-1, nullptr, VP_FP16X3, gpu_id);
    const DevPlanes d = upload_planes(g, hi, lo, (size_t)h * w * c_pitch);
    unsigned long long* dr = reinterpret_cast<unsigned long long*>(g.alloc_f32(2 * vp::VP_HIST_WORDS));   // zeroed
    VP_HIP_CHECK(vp::launch_act_exp_hist(d.hi, d.lo, c, h, w, c_pitch, dr, g.stream()));
    unsigned long long r[vp::VP_HIST_WORDS];
    g.copy_d2h(r, dr, sizeof(r));
    std::memcpy(bins, r, VP_RANGE_BINS * sizeof(unsigned long long));
    *zeros = r[VP_RANGE_BINS];
    *count = r[VP_RANGE_BINS + 1];
  });
}

int vp_op_conv2d_scaled(int gpu_id, int precision, int mode, const float* in, int cin, int h, int w, const float* weight, const float* bias, int cout, int ks,
                        int act, int res_mode, const float* res, int tile, int bk, int nsplit, int in_exp, int res_exp, int out_exp, uint16_t* out_hi,
                        uint16_t* out_lo, char* err, size_t err_len) {
  return op_guarded(err, err_len, [&] {
    if (!in || !weight || !bias || !out_hi || cin < 1 || cout < 1 || h < 1 || w < 1 || (long long)h * w > (1 << 20)) throw std::invalid_argument("bad argument");
    if (mode != 0) throw std::invalid_argument("vp_op_conv2d_scaled: mode 0 (Conv2d) only");
    vp::Engine g(-1, nullptr, precision | VP_ACT_SCALE, gpu_id);
    vp::Act* a = g.new_act("in", cin, h, w);
    upload_act_scaled(g, a, in, in_exp);
    g.set_act_exp(a, in_exp);
    vp::ConvOpts o;
    o.act = act;
    o.tile = tile;
    o.bk = bk;
    o.nsplit = nsplit;
    if (res_mode != 0) {
      if (!res) throw std::invalid_argument("res_mode set but res is null");
      vp::Act* r = g.new_act("res", cout, h, w);
      upload_act_scaled(g, r, res, res_exp);
      g.set_act_exp(r, res_exp);
      o.res_mode = res_mode;
      o.res = r;
    }
    const size_t wn = (size_t)cin * cout * ks * ks;
    vp::Act* y = g.add_conv("op", a, std::vector<float>(weight, weight + wn), std::vector<float>(bias, bias + cout), cout, ks, o);
    g.set_act_exp(y, out_exp);
    g.run_eager();
    g.sync();
    read_planes_chw(g, y, out_hi, out_lo);
  });
}

// ---- the convolution forms the networks launch beyond vp_op_conv2d's (unit tests): stride 2, activation behind the residual, alias-slice
// destination, residual read from a slice, all of them with or without exponents -- through add_conv, as the plan builders do
int vp_op_conv2d_forms(int gpu_id, int precision, const vp_conv_form* form, const float* in, const float* weight, const float* bias, const float* res,
                       const float* dst_init, uint16_t* out_hi, uint16_t* out_lo, char* err, size_t err_len) {
  return op_guarded(err, err_len, [&] {
    if (!form || !in || !weight || !bias || !out_hi) throw std::invalid_argument("bad argument");
    const vp_conv_form& f = *form;
    if (f.cin < 1 || f.cout < 1 || f.h < 1 || f.w < 1 || (long long)f.h * f.w > (1 << 20) || (f.ks != 1 && f.ks != 3) || (f.stride != 1 && f.stride != 2) || f.res_mode < 0 ||
        f.res_mode > 2 || f.res_where < 0 || f.res_where > 1 || f.res_h < 0 || f.res_w < 0 || (long long)f.res_h * f.res_w > (1 << 20))
      throw std::invalid_argument("bad argument (ks 1 or 3, stride 1 or 2, res_mode 0 .. 2, res_where 0 or 1)");
    if (f.dst_c != 0 && (f.dst_c < 32 || (f.dst_c & 31) || f.dst_off < 0 || (f.dst_off & 31) || (f.cout & 31) || f.dst_off + f.cout > f.dst_c))
      throw std::invalid_argument("bad argument (dst_c, dst_off, cout: multiples of 32 with dst_off + cout <= dst_c)");
    if (f.res_mode != 0 && f.res_where == 1 && (f.dst_c == 0 || f.res_off < 0 || (f.res_off & 31) || f.res_off + f.cout > f.dst_c))
      throw std::invalid_argument("bad argument (res_where 1: a slice destination, res_off a multiple of 32 with res_off + cout <= dst_c)");
    if (f.res_mode != 0 && f.res_where == 0 && !res) throw std::invalid_argument("res_mode set but res is null");
    if (f.in_c != 0 && (f.in_c < 32 || (f.in_c & 31) || f.in_off < 0 || (f.in_off & 31) || (f.cin & 31) || f.in_off + f.cin > f.in_c))
      throw std::invalid_argument("bad argument (in_c, in_off, cin: multiples of 32 with in_off + cin <= in_c)");
    const bool scaled = (f.in_exp | f.res_exp | f.out_exp) != 0 || (precision & VP_ACT_SCALE) != 0;   // the flag alone: a flagged engine with every exponent 0
    vp::Engine g(-1, nullptr, precision | (scaled ? VP_ACT_SCALE : 0), gpu_id);
    const int oh = f.h / f.stride, ow = f.w / f.stride;
    const vp::Act* a;
    if (f.in_c != 0) {   // only ever refused (add_conv): nothing is uploaded
      a = g.alias_slice("in", g.new_act("in.whole", f.in_c, f.h, f.w), f.in_off, f.cin);
    } else {
      vp::Act* t = g.new_act("in", f.cin, f.h, f.w);
      upload_act_scaled(g, t, in, f.in_exp);
      if (scaled) g.set_act_exp(t, f.in_exp);
      a = t;
    }
    vp::Act* dst = nullptr;
    if (f.dst_c != 0) {
      dst = g.new_act("dst", f.dst_c, oh, ow);
      if (dst_init) upload_act_scaled(g, dst, dst_init, f.out_exp);
      if (scaled) g.set_act_exp(dst, f.out_exp);   // its alias slices share the exponent
    }
    vp::ConvOpts o;
    o.act = f.act;
    o.post_act = f.post_act;
    o.stride = f.stride;
    o.tile = f.tile;
    o.bk = f.bk;
    o.nsplit = f.nsplit;
    if (f.res_mode != 0) {
      o.res_mode = f.res_mode;
      if (f.res_where == 1) {
        o.res = g.alias_slice("res", dst, f.res_off, f.cout);
      } else {
        vp::Act* r = g.new_act("res", f.cout, f.res_h > 0 ? f.res_h : oh, f.res_w > 0 ? f.res_w : ow);
        upload_act_scaled(g, r, res, f.res_exp);
        if (scaled) g.set_act_exp(r, f.res_exp);
        o.res = r;
      }
    }
    const size_t wn = (size_t)f.cin * f.cout * f.ks * f.ks;
    vp::Act* y = g.add_conv("op", a, std::vector<float>(weight, weight + wn), std::vector<float>(bias, bias + f.cout), f.cout, f.ks, o,
                            dst ? g.alias_slice("op", dst, f.dst_off, f.cout) : nullptr);
    if (scaled && !dst) g.set_act_exp(y, f.out_exp);
    g.run_eager();
    g.sync();
    read_planes_chw(g, dst ? dst : y, out_hi, out_lo);
  });
}

// ---- single-operator entries of the AutoSteer head's kernels (unit tests)
int vp_op_rowpair_conv(int gpu_id, int precision, const float* in, int cin, int h, int w, const float* weight, const float* bias, int replicate,
                       int dst_c, int dst_off, const float* dst_init, uint16_t* out_hi, uint16_t* out_lo, char* err, size_t err_len) {
  return op_guarded(err, err_len, [&] { op_rowpair_conv(gpu_id, precision, in, cin, h, w, weight, bias, replicate, dst_c, dst_off, dst_init, 0, 0, out_hi, out_lo); });
}

int vp_op_lane_rows_head(int gpu_id, int precision, const float* features, int cin, int h, int w, const float* c1_w, float c1_b, const float* c2_w,
                         float c2_b, const float* h1_w, float h1_b, const float* h2_w, float h2_b, float* out_2xh, char* err, size_t err_len) {
  return op_guarded(err, err_len, [&] { op_lane_rows_head(gpu_id, precision, features, cin, h, w, c1_w, c1_b, c2_w, c2_b, h1_w, h1_b, h2_w, h2_b, 0, out_2xh); });
}

// ---- the detector's and the lane network's own kernels under VP_ACT_SCALE (unit tests): arguments are TRUE values, stored as x * 2^-exp
int vp_op_upsample2_cat_scaled(int gpu_id, int precision, const float* a, int ca, int a_off, int a_nch, const float* b, int cb, int b_off, int b_nch, int h, int w,
                               int exp, uint16_t* out_hi, uint16_t* out_lo, char* err, size_t err_len) {
  return op_guarded(err, err_len, [&] {
    if (!a || !b || !out_hi || ca < 1 || cb < 1 || h < 1 || w < 1 || (long long)h * w > (1 << 20) || a_nch < 8 || b_nch < 8 || ((a_off | a_nch | b_off | b_nch) & 7) || a_off < 0 ||
        b_off < 0 || a_off + a_nch > ca || b_off + b_nch > cb)
      throw std::invalid_argument("bad argument (offsets and widths: multiples of 8 inside the sources)");
    vp::Engine g(-1, nullptr, precision | VP_ACT_SCALE, gpu_id);
    vp::Act* ta = g.new_act("a", ca, h, w);
    vp::Act* tb = g.new_act("b", cb, 2 * h, 2 * w);
    vp::Act* to = g.new_act("out", a_nch + b_nch, 2 * h, 2 * w);
    upload_act_scaled(g, ta, a, exp);
    upload_act_scaled(g, tb, b, exp);
    g.add_up_cat("op", ta, tb, to, a_off, a_nch, b_off, b_nch);   // ties a, b and out: a mover keeps the exponent
    g.set_act_exp(to, exp);
    if (g.act_exp(ta) != exp || g.act_exp(tb) != exp) throw std::runtime_error("upsample2_cat: the sources do not carry the result's exponent");
    g.run_eager();
    g.sync();
    read_planes_chw(g, to, out_hi, out_lo);
  });
}

int vp_op_detect_head_decode_scaled(int gpu_id, int precision, const float* box, const float* cls, int nc, int h0, int w0, const int* exps, float* out, char* err,
                                    size_t err_len) {
  return op_guarded(err, err_len, [&] {
    if (!exps) throw std::invalid_argument("bad argument (exps: six exponents, box and cls of the three levels)");
    op_detect_head_decode(gpu_id, precision, box, cls, nc, h0, w0, exps, out);
  });
}

int vp_op_rowpair_conv_scaled(int gpu_id, int precision, const float* in, int cin, int h, int w, const float* weight, const float* bias, int replicate, int dst_c,
                              int dst_off, const float* dst_init, int in_exp, int out_exp, uint16_t* out_hi, uint16_t* out_lo, char* err, size_t err_len) {
  return op_guarded(err, err_len, [&] {
    op_rowpair_conv(gpu_id, precision, in, cin, h, w, weight, bias, replicate, dst_c, dst_off, dst_init, in_exp, out_exp, out_hi, out_lo);
  });
}

int vp_op_lane_rows_head_scaled(int gpu_id, int precision, const float* features, int cin, int h, int w, const float* c1_w, float c1_b, const float* c2_w,
                                float c2_b, const float* h1_w, float h1_b, const float* h2_w, float h2_b, int in_exp, float* out_2xh, char* err, size_t err_len) {
  return op_guarded(err, err_len, [&] {
    op_lane_rows_head(gpu_id, precision, features, cin, h, w, c1_w, c1_b, c2_w, c2_b, h1_w, h1_b, h2_w, h2_b, in_exp, out_2xh);
  });
}

// ---- composed up-sampling stage (round 6): the load-time weight composition alone, and the whole stage as one operator
int vp_compose_upconv(int gpu_id, const float* wt, const float* bt, const float* ws, const float* bs, const float* w3, const float* b3, int cin, int cm,
                      int cout, int cs, double* wx, double* wsk, double* bias, char* err, size_t err_len) {
  return op_guarded(err, err_len, [&] {
    if (!wt || !bt || !w3 || !b3 || !wx || !bias || cin < 1 || cm < 1 || cout < 1 || cs < 0 || (cs > 0 && (!ws || !bs || !wsk))) throw std::invalid_argument("bad argument");
    vp::Engine g(-1, nullptr, VP_FP16X3, gpu_id);
    vp::UpconvComposed c;
    g.compose_upconv(wt, bt, ws, bs, w3, b3, cin, cm, cout, cs, &c);
    std::memcpy(wx, c.wx.data(), c.wx.size() * sizeof(double));
    if (cs > 0) std::memcpy(wsk, c.ws.data(), c.ws.size() * sizeof(double));
    std::memcpy(bias, c.bias.data(), c.bias.size() * sizeof(double));
  });
}

// ---- vp_frame's rectification kernel on a host picture through any map (unit tests)
int vp_op_remap_bgr8(int gpu_id, const uint8_t* src, int src_h, int src_w, int src_stride, const int16_t* xy, const uint16_t* frac, int out_h, int out_w,
                     int border, uint8_t* dst, int dst_stride, char* err, size_t err_len) {
  return op_guarded(err, err_len, [&] {
    if (!src || !xy || !frac || !dst || src_h < 1 || src_w < 1 || src_h > 16384 || src_w > 16384 || out_h < 1 || out_w < 1 || out_h > 16384 || out_w > 16384 ||
        src_stride < 3 * src_w || dst_stride < 3 * out_w || (border != VP_BORDER_CONSTANT && border != VP_BORDER_REPLICATE))
      throw std::invalid_argument("vp_op_remap_bgr8: bad argument (sizes 1 .. 16384, strides of at least 3 * width, border VP_BORDER_CONSTANT / VP_BORDER_REPLICATE)");
    const size_t n = (size_t)out_h * out_w;
    const int mp = vp::frame_remap_map_pitch(out_w);
    std::vector<vp::RemapEntry> m((size_t)out_h * mp, vp::RemapEntry{0, 0});
    for (size_t i = 0; i < n; ++i) {
      if (frac[i] >= 1024) throw std::invalid_argument("vp_op_remap_bgr8: frac = fy << 5 | fx with fx, fy below 32");
      m[(i / out_w) * mp + i % out_w] = {(int)xy[2 * i] * 32 + (frac[i] & 31), (int)xy[2 * i + 1] * 32 + (frac[i] >> 5)};
    }
    vp::Engine g(-1, nullptr, VP_FP16X3, gpu_id);
    const size_t src_bytes = (size_t)(src_h - 1) * src_stride + (size_t)3 * src_w;
    const int pitch = vp::frame_bgr_pitch(out_w);
    const size_t dst_bytes = (size_t)out_h * pitch;
    uint8_t* d_src = reinterpret_cast<uint8_t*>(g.alloc_f32((src_bytes + 3) / 4));
    vp::RemapEntry* d_map = reinterpret_cast<vp::RemapEntry*>(g.alloc_f32(2 * m.size()));
    uint8_t* d_dst = reinterpret_cast<uint8_t*>(g.alloc_f32(dst_bytes / 4));
    g.copy_h2d(d_src, src, src_bytes);
    g.copy_h2d(d_map, m.data(), m.size() * sizeof(vp::RemapEntry));
    VP_HIP_CHECK(hipMemsetAsync(d_dst, 0xFF, dst_bytes, g.stream()));
    vp::FrameRemapParams q{};
    q.src = d_src;
    q.src_pitch = src_stride;
    q.src_h = src_h;
    q.src_w = src_w;
    q.map = d_map;
    q.map_pitch = mp;
    q.border = border;
    q.dst = d_dst;
    q.dst_pitch = pitch;
    q.out_h = out_h;
    q.out_w = out_w;
    VP_HIP_CHECK(vp::launch_frame_remap(q, g.stream()));
    std::vector<uint8_t> back(dst_bytes);
    g.copy_d2h(back.data(), d_dst, dst_bytes);
    const size_t row = (size_t)(dst_stride >= pitch ? pitch : 3 * out_w);
    for (int y = 0; y < out_h; ++y) std::memcpy(dst + (size_t)y * dst_stride, back.data() + (size_t)y * pitch, row);
  });
}

// ---- the canvas's JPEG encoder on a host picture, and its host half (no device)
int vp_op_jpeg_encode_bgr8(int gpu_id, const uint8_t* bgr, int h, int w, int stride, int quality, int restart_mcus, uint8_t* dst, size_t cap, size_t* n, char* err,
                           size_t err_len) {
  return op_guarded(err, err_len, [&] {
    if (!bgr || !dst || !n) throw std::invalid_argument("vp_op_jpeg_encode_bgr8: null bgr / dst / n");
    check_jpeg_args("vp_op_jpeg_encode_bgr8", h, w, quality, restart_mcus);
    if (stride < 3 * w) throw std::invalid_argument("vp_op_jpeg_encode_bgr8: stride " + std::to_string(stride) + " is below the row's " + std::to_string(3 * w) + " bytes");
    vp::Engine g(-1, nullptr, VP_FP16X3, gpu_id);
    const int pitch = vp::frame_bgr_pitch(w);
    uint8_t* d_src = reinterpret_cast<uint8_t*>(g.alloc_f32((size_t)h * pitch / 4));
    std::vector<uint8_t> rows((size_t)h * pitch, 0);   // the canvas's own layout: bytes behind a row's end are 0
    for (int y = 0; y < h; ++y) std::memcpy(rows.data() + (size_t)y * pitch, bgr + (size_t)y * stride, (size_t)3 * w);
    g.copy_h2d(d_src, rows.data(), rows.size());
    vp::JpegEncoder enc;
    enc.encode(d_src, pitch, h, w, quality, restart_mcus, dst, cap, n, "vp_op_jpeg_encode_bgr8", g.stream());
  });
}

int vp_jpeg_bound(int h, int w, int restart_mcus, size_t* bytes, char* err, size_t err_len) {
  return op_guarded(err, err_len, [&] {
    if (!bytes) throw std::invalid_argument("vp_jpeg_bound: null bytes");
    check_jpeg_args("vp_jpeg_bound", h, w, 100, restart_mcus);
    *bytes = vp::jpeg_bound(h, w, restart_mcus);
  });
}

int vp_jpeg_header(int h, int w, int quality, int restart_mcus, uint8_t* dst, size_t cap, size_t* n, char* err, size_t err_len) {
  return op_guarded(err, err_len, [&] {
    if (!dst || !n) throw std::invalid_argument("vp_jpeg_header: null dst / n");
    check_jpeg_args("vp_jpeg_header", h, w, quality, restart_mcus);
    if (cap < vp::kJpegHeaderBytes) {
      *n = vp::kJpegHeaderBytes;
      throw std::invalid_argument("vp_jpeg_header: the header has " + std::to_string(vp::kJpegHeaderBytes) + " bytes, cap is " + std::to_string(cap));
    }
    vp::jpeg_write_header(h, w, quality, restart_mcus, dst);
    *n = vp::kJpegHeaderBytes;
  });
}

int vp_op_upconv(int gpu_id, const float* in, int cin, int h, int w, const float* skip, int cs, const float* wt, const float* bt, const float* ws,
                 const float* bs, const float* w3, const float* b3, int cm, int cout, int act, int shape, int nsplit, int precision, float* out, char* err,
                 size_t err_len) {
  return op_guarded(err, err_len, [&] {
    if (precision != VP_FP16 && precision != VP_FP16X3) throw std::invalid_argument("precision must be VP_FP16 or VP_FP16X3");
    if (!in || !wt || !bt || !w3 || !b3 || !out || cin < 1 || cm < 1 || cout < 1 || h < 1 || w < 1 || cs < 0 || (cs > 0 && (!skip || !ws || !bs)))
      throw std::invalid_argument("bad argument");
    vp::Engine g(-1, nullptr, precision, gpu_id);
    vp::Act* a = g.new_act("in", cin, h, w);
    g.upload_act(a, in);
    vp::Act* sk = nullptr;
    if (cs > 0) {
      sk = g.new_act("skip", cs, 2 * h, 2 * w);
      g.upload_act(sk, skip);
    }
    const std::vector<float> vwt(wt, wt + (size_t)cin * cm * 4), vbt(bt, bt + cm), vw3(w3, w3 + (size_t)cout * cm * 9), vb3(b3, b3 + cout);
    const std::vector<float> vws(cs > 0 ? ws : nullptr, cs > 0 ? ws + (size_t)cm * cs : nullptr), vbs(cs > 0 ? bs : nullptr, cs > 0 ? bs + cm : nullptr);
    vp::Act* y = g.add_upconv("op", a, sk, vwt, vbt, vws, vbs, vw3, vb3, cm, cout, act, shape, nsplit);
    g.run_eager();
    g.sync();
    read_act_chw(g, y, out);
  }, VP_ERR_RANGE);
}

// ---- vp_metric's radix select alone (unit tests)
int vp_op_select_f32(int gpu_id, const float* values, int n, int k, float* out, char* err, size_t err_len) {
  return op_guarded(err, err_len, [&] {
    if (!values || !out || n < 1 || n > (int)vp::kMetricMaxN || k < 0 || k >= n) throw std::invalid_argument("vp_op_select_f32: bad argument (n 1 .. 2^24, k 0 .. n - 1)");
    std::vector<unsigned> bits((size_t)n);
    std::memcpy(bits.data(), values, (size_t)n * sizeof(float));
    for (int i = 0; i < n; ++i)
      if (bits[i] >= 0x7F800000u) throw std::invalid_argument("vp_op_select_f32: value " + std::to_string(i) + " is negative or not finite");
    vp::Engine g(-1, nullptr, VP_FP16X3, gpu_id);
    unsigned* d_bits = reinterpret_cast<unsigned*>(g.alloc_f32((size_t)n));
    unsigned* d_out = reinterpret_cast<unsigned*>(g.alloc_f32(2));
    unsigned* d_scratch = reinterpret_cast<unsigned*>(g.alloc_f32(vp::metric_select_scratch_bytes((unsigned)n) / sizeof(float)));
    g.copy_h2d(d_bits, bits.data(), (size_t)n * sizeof(unsigned));
    VP_HIP_CHECK(vp::launch_metric_select(d_bits, (unsigned)n, (unsigned)k, (unsigned)k, d_scratch, d_out, g.stream()));
    unsigned got[2];
    g.copy_d2h(got, d_out, sizeof(got));
    std::memcpy(out, got, sizeof(float));
  });
}

// ---- the detector validation's candidate / rank / suppression chain alone (unit tests)
int vp_op_detect_validate(int gpu_id, const float* raw, int nc, int nb, float conf, float iou, float* rows_out, int cap, uint32_t* counts_out, char* err, size_t err_len) {
  return op_guarded(err, err_len, [&] {
    if (!raw || !counts_out || cap < 0 || (cap > 0 && !rows_out) || nc < 1 || nc > vp::kDetValMaxClasses || nb < 1 || nb > vp::kDetValMaxBoxes ||
        (long long)nb * nc > (long long)vp::kDetValMaxPairs || conf != conf || iou != iou)
      throw std::invalid_argument("vp_op_detect_validate: bad argument (nc 1 .. 80, nb 1 .. 16384, nb * nc <= 131072, thresholds not NaN)");
    vp::Engine g(-1, nullptr, VP_FP16X3, gpu_id);
    const size_t words = (size_t)(4 + nc) * nb;
    float* d_raw = g.alloc_f32(words);
    uint8_t* d_scratch = reinterpret_cast<uint8_t*>(g.alloc_f32(vp::det_val_scratch_bytes((unsigned)nb, (unsigned)nc) / sizeof(float)));
    float* d_rows = g.alloc_f32((size_t)vp::kDetValMaxDet * vp::kDetValRowWords);
    unsigned* d_counts = reinterpret_cast<unsigned*>(g.alloc_f32(4));
    g.copy_h2d(d_raw, raw, words * sizeof(float));
    vp::DetValParams q{};
    q.raw = d_raw;
    q.nb = (unsigned)nb;
    q.nc = (unsigned)nc;
    q.conf = conf;
    q.iou = iou;
    q.max_nms = vp::kDetValMaxNms;
    q.max_det = vp::kDetValMaxDet;
    vp::det_val_carve(d_scratch, &q);
    q.rows = d_rows;
    q.counts = d_counts;
    VP_HIP_CHECK(vp::launch_det_validate(q, g.stream()));
    unsigned counts[3];
    g.copy_d2h(counts, d_counts, sizeof(counts));
    for (int i = 0; i < 3; ++i) counts_out[i] = counts[i];
    const size_t n = std::min((size_t)cap, (size_t)counts[2]);
    if (n) {
      std::vector<float> rows((size_t)counts[2] * vp::kDetValRowWords);
      g.copy_d2h(rows.data(), d_rows, rows.size() * sizeof(float));
      for (size_t r = 0; r < n; ++r) std::memcpy(rows_out + r * 6, rows.data() + r * vp::kDetValRowWords, 6 * sizeof(float));
    }
  });
}

// ---- vp_metric's label kernels alone: host label in, host ground truth and record out
namespace {
int* op_label_tab(vp::Engine& g, int src, int dst) {
  std::vector<int> tab((size_t)dst);
  vp::label_nearest_tab(src, dst, tab.data());
  int* d = reinterpret_cast<int*>(g.alloc_f32((size_t)dst));
  g.copy_h2d(d, tab.data(), tab.size() * sizeof(int));
  return d;
}
void op_label_out_dims(const char* who, const void* gt_out, const void* frame_out, int oh, int ow) {
  if (!gt_out || !frame_out) throw std::invalid_argument(std::string(who) + ": null output");
  if (oh < 1 || ow < 1 || (long long)oh * ow > (long long)vp::kMetricMaxN) throw std::invalid_argument(std::string(who) + ": oh * ow outside 1 .. 2^24");
}
}  // namespace

int vp_op_label_gt(int gpu_id, const uint8_t* label, int channels, int h, int w, int stride_bytes, const int* crop_ltrb, const uint8_t* colours, int n_colours, int oh, int ow,
                   uint8_t* gt_out, vp_label_frame* frame_out, char* err, size_t err_len) {
  return op_guarded(err, err_len, [&] {
    vp::LabelSegParams q = vp::label_seg_params("vp_op_label_gt", label, channels, h, w, stride_bytes, crop_ltrb, colours, n_colours);
    op_label_out_dims("vp_op_label_gt", gt_out, frame_out, oh, ow);
    vp::Engine g(-1, nullptr, VP_FP16X3, gpu_id);
    const size_t bytes = (size_t)(h - 1) * stride_bytes + (size_t)w * channels, n_out = (size_t)oh * ow;
    uint8_t* d_label = reinterpret_cast<uint8_t*>(g.alloc_f32((bytes + 3) / 4));
    g.copy_h2d(d_label, label, bytes);
    q.label = d_label;
    q.ty = op_label_tab(g, q.ch, oh);
    q.tx = op_label_tab(g, q.cw, ow);
    q.oh = oh;
    q.ow = ow;
    q.gt = reinterpret_cast<uint8_t*>(g.alloc_f32((n_out + 3) / 4));
    q.part = reinterpret_cast<unsigned*>(g.alloc_f32(4 * (size_t)vp::kMetricBlocks));
    q.rec = reinterpret_cast<vp::LabelRecord*>(g.alloc_f32(sizeof(vp::LabelRecord) / sizeof(float)));
    VP_HIP_CHECK(vp::launch_label_seg(q, g.stream()));
    g.copy_d2h(gt_out, q.gt, n_out);
    g.copy_d2h(frame_out, q.rec, sizeof(vp::LabelRecord));
  });
}

int vp_op_label_depth_gt(int gpu_id, const void* label, int dtype, int h, int w, int stride_elems, int oh, int ow, float* gt_out, vp_label_frame* frame_out, char* err,
                         size_t err_len) {
  return op_guarded(err, err_len, [&] {
    vp::label_check_depth("vp_op_label_depth_gt", label, dtype, h, w, stride_elems);
    op_label_out_dims("vp_op_label_depth_gt", gt_out, frame_out, oh, ow);
    vp::Engine g(-1, nullptr, VP_FP16X3, gpu_id);
    const size_t es = dtype == VP_LABEL_F64 ? sizeof(double) : sizeof(float), bytes = es * ((size_t)(h - 1) * stride_elems + (size_t)w), n_out = (size_t)oh * ow;
    void* d_label = g.alloc_f32(bytes / sizeof(float));
    g.copy_h2d(d_label, label, bytes);
    vp::LabelDepthParams q{};
    q.label = d_label;
    q.dtype = dtype;
    q.h = h;
    q.w = w;
    q.stride = stride_elems;
    q.ty = op_label_tab(g, h, oh);
    q.tx = op_label_tab(g, w, ow);
    q.oh = oh;
    q.ow = ow;
    q.gt = g.alloc_f32(n_out);
    q.part = reinterpret_cast<vp::LabelExtPartial*>(g.alloc_f32((size_t)vp::kMetricBlocks * sizeof(vp::LabelExtPartial) / sizeof(float)));
    q.rec = reinterpret_cast<vp::LabelRecord*>(g.alloc_f32(sizeof(vp::LabelRecord) / sizeof(float)));
    VP_HIP_CHECK(vp::launch_label_depth(q, g.stream()));
    g.copy_d2h(gt_out, q.gt, n_out * sizeof(float));
    g.copy_d2h(frame_out, q.rec, sizeof(vp::LabelRecord));
  });
}

}  // extern "C"

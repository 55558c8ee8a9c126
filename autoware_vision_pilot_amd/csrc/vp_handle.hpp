// The opaque handles behind include/vp_hip.h (shared by vp_api.cpp, vp_detect.cpp and vp_comm.cpp).
#pragma once
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/vp_hip.h"
#include "engine.hpp"

struct vp_engine {
  std::unique_ptr<vp::Engine> impl;
  std::string err;
};

// vp_frame: one camera frame, uploaded once in its native format and kept as packed BGR8 on the device for any number of consumers (engines, the
// detector).  Owns its stream and buffers; the member functions are defined in vp_api.cpp.
// Ordering, all of it on the device: an upload ends with `ready` recorded on the frame's stream, and every consumer's stream waits for that event
// ahead of its region copy; a consumer records its own event behind the copy (note_consumer), and the next upload makes the frame's stream wait for
// every such event before it overwrites the image (wait_for_consumers).  `consumers` is the only state two threads touch: consumers on different
// engines may run concurrently, so it sits behind `mu`.  One event per consumer stream is enough: a later record on the same stream lies behind the
// earlier copy too.
struct vp_frame {
  int gpu = 0;
  hipStream_t stream = nullptr;
  uint8_t* d_bgr = nullptr;      // [h][pitch], pitch = vp::frame_bgr_pitch(w)
  size_t bgr_cap = 0;
  uint8_t* d_src = nullptr;      // the native planes of a host upload, rows packed, plane after plane (what the conversion kernel reads)
  size_t src_cap = 0;
  uint8_t* h_stage = nullptr;    // pinned staging of a pageable host frame: two slots, as the engines' (engine_io.cpp upload_frame)
  size_t stage_cap = 0;          // bytes per slot
  int stage_slot = 0;
  hipEvent_t stage_ev[2] = {nullptr, nullptr};
  int h = 0, w = 0, pitch = 0;
  bool uploaded = false;
  int color_matrix = 0, color_range = 0;   // vp_frame_set_color: the standard of later YUV uploads (BT.601, limited range)
  // vp_frame_set_raw: the setting of later Bayer uploads (raw.lut stays null: the table lives in d_lut, raw.lut_len entries of it, copied on the
  // frame's stream at the call, behind every conversion queued before it)
  vp_raw raw{0, 0, 0, {256, 256, 256}, 0, {0, 0, 0, 0, 0, 0, 0, 0, 0}, nullptr, 0};
  uint8_t* d_lut = nullptr;      // [4096]
  // vp_frame_set_rectify: later uploads convert into d_raw (the camera's geometry) and are resampled into d_bgr (the standard pose's) on the frame's
  // stream, ahead of `ready`.  Maps: built on the host once per (raw geometry, setting), kept on the device; d_map[0] undistort or the one-pass map,
  // d_map[1] the warp (an identity pass has no map and is skipped).
  bool rect_on = false;
  vp_rectify rect{};
  uint8_t* d_raw = nullptr;      // [raw h][frame_bgr_pitch(raw w)]: what the conversion writes while rectification is on
  size_t raw_cap = 0;
  uint8_t* d_mid = nullptr;      // the undistorted picture between the two passes, raw geometry
  size_t mid_cap = 0;
  vp::RemapEntry* d_map[2] = {nullptr, nullptr};
  size_t map_cap[2] = {0, 0};
  int map_h = 0, map_w = 0;      // the raw geometry the maps were built for; 0: none (the setting changed)
  hipEvent_t ready = nullptr;     // content complete
  hipEvent_t producer = nullptr;  // vp_frame_upload_device: recorded on the caller's producer stream
  struct Consumer {
    hipStream_t stream;
    hipEvent_t done;
    bool pending;
  };
  std::mutex mu;
  std::vector<Consumer> consumers;
  std::string err;

  ~vp_frame();
  vp::FrameView view() const;
  void note_consumer(hipStream_t s);   // behind a consumer's copy, on the consumer's stream
  void wait_for_consumers();           // ahead of an upload, on the frame's stream
};

// vp_canvas: one picture per camera frame, composed on the device (vp::Canvas, engine.hpp / engine_io.cpp; C ABI: vp_api.cpp).  One thread drives it.
struct vp_canvas {
  std::unique_ptr<vp::Canvas> impl;
  std::string err;
};

// vp_metric: the validation scores of the reference's trainers, one record per frame on the device (vp::Metric, engine.hpp / engine_io.cpp; C ABI:
// vp_api.cpp).  `host`: the records of the last fetch, from which the summary is formed.  One thread drives it.
struct vp_metric {
  std::unique_ptr<vp::Metric> impl;
  std::vector<vp_metric_frame> host;
  // the detector part's last fetch: frame records, kept rows and label classes
  std::vector<vp::DetFrameRecord> det_frames;
  std::vector<vp::DetRowRecord> det_rows;
  std::vector<float> det_label_cls;
  std::string err;
};

// vp_lanes: the production lane filter behind an EgoLanes pass (vp::Lanes, engine.hpp / engine_io.cpp; C ABI: vp_api.cpp).  `recs` / `fits`: the
// scratch of a fetch.  One thread drives it.
struct vp_lanes {
  std::unique_ptr<vp::Lanes> impl;
  std::vector<vp::LaneFilterRecord> recs;
  std::vector<vp::LanesFit> fits;
  std::string err;
};

// LaneFilterHip -- what autoware_pov::vision::egolanes::LaneFilter::update (VisionPilot/production_release/src/lane_filtering/lane_filter.cpp) hands the
// lateral thread, computed on the device behind the EgoLanes pass (vp_lanes, include/vp_hip.h): the logits never leave the GPU, one record of about
// 1 KB does.  In production_release/main.cpp:505-545
//     LaneSegmentation raw_lanes = engine.inference(frame, threshold);
//     LaneSegmentation filtered_lanes = lane_filter.update(raw_lanes);
// becomes
//     LaneSegmentation filtered_lanes = lane_filter_hip.update(frame, engine, threshold);      // or engine.enqueue(frame); lane_filter_hip.update(engine, threshold);
// and LaneTracker::update consumes `filtered_lanes` unchanged: width, height, left_coeffs / right_coeffs (six numbers, or empty when the lane has no
// fit this frame), the start points and the sliding windows.  The three masks stay empty unless with_masks is set (the display path's
// drawRawMasksInPlace wants them; vp_canvas_overlay_lanes draws them on the device instead).
// Departures from the reference, both stated in include/vp_hip.h: its RANSAC loop is a no-op and is not run; a singular system gives no fit where
// cv::solve(DECOMP_SVD) would answer the minimum-norm solution.
#ifndef LANE_FILTER_HIP_HPP_
#define LANE_FILTER_HIP_HPP_

#include <stdexcept>
#include <string>

#include "egolanes_hip_engine.hpp"
#include "inference/lane_segmentation.hpp"  // the reference's LaneSegmentation
#include "vp_hip.h"

namespace autoware_pov::vision::egolanes
{

class LaneFilterHip
{
public:
  explicit LaneFilterHip(float smoothing_factor = 0.5f, int device_id = 0)
  {
    char err[512] = {0};
    if (vp_lanes_create(&lanes_, device_id, 4, err, sizeof(err)) != VP_OK) throw std::runtime_error(std::string("[lane_filter_hip] ") + err);
    if (vp_lanes_set_smoothing(lanes_, smoothing_factor) != VP_OK) {
      const std::string msg = vp_lanes_last_error(lanes_);
      vp_lanes_destroy(lanes_);
      throw std::runtime_error("[lane_filter_hip] " + msg);
    }
  }
  ~LaneFilterHip() { vp_lanes_destroy(lanes_); }
  LaneFilterHip(const LaneFilterHip &) = delete;
  LaneFilterHip & operator=(const LaneFilterHip &) = delete;

  // the engine has a pass queued or finished (EgoLanesHipEngine::enqueue / inference); an empty LaneSegmentation{} on failure, as the engines answer
  LaneSegmentation update(EgoLanesHipEngine & engine, float threshold = 0.0f, bool with_masks = false)
  {
    vp_lanes_result r;
    int n = 0;
    if (vp_lanes_add(lanes_, engine.handle(), threshold) != VP_OK || vp_lanes_fetch(lanes_, &r, 1, &n) != VP_OK || n != 1) return LaneSegmentation{};
    LaneSegmentation out;
    if (with_masks && !masks(engine.handle(), threshold, out)) return LaneSegmentation{};
    out.width = 160;
    out.height = 80;
    fill(r.lane[0], out.left_coeffs, out.left_start_point, out.left_sliding_windows);
    fill(r.lane[1], out.right_coeffs, out.right_start_point, out.right_sliding_windows);
    last_ = r;
    return out;
  }
  LaneSegmentation update(const cv::Mat & frame, EgoLanesHipEngine & engine, float threshold = 0.0f, bool with_masks = false)
  {
    if (!engine.enqueue(frame)) return LaneSegmentation{};
    return update(engine, threshold, with_masks);
  }
  void reset()
  {
    if (vp_lanes_reset(lanes_) != VP_OK) throw std::runtime_error(std::string("[lane_filter_hip] ") + vp_lanes_last_error(lanes_));
  }
  // the last record as the library gave it: point counts, moments, order, flags, this frame's own fit
  const vp_lanes_result & lastRecord() const { return last_; }

private:
  // postProcess of the reference's engines (onnxruntime_engine.cpp:151-192): three CV_32FC1 0/1 planes, '> threshold'; this is the full D2H the
  // filter otherwise avoids
  static bool masks(vp_engine * e, float threshold, LaneSegmentation & out)
  {
    const float * raw = nullptr;
    int64_t shape[4];
    if (vp_fetch_outputs(e) != VP_OK || vp_logits(e, &raw, shape) != VP_OK) return false;
    const int h = static_cast<int>(shape[2]), w = static_cast<int>(shape[3]), n = h * w;
    cv::Mat * planes[3] = {&out.ego_left, &out.ego_right, &out.other_lanes};
    for (int c = 0; c < 3; ++c) {
      planes[c]->create(h, w, CV_32FC1);
      float * dst = reinterpret_cast<float *>(planes[c]->data);
      const float * src = raw + static_cast<size_t>(c) * n;
      for (int i = 0; i < n; ++i) dst[i] = src[i] > threshold ? 1.0f : 0.0f;
    }
    return true;
  }
  static void fill(const vp_lanes_lane & l, std::vector<double> & coeffs, cv::Point & start, std::vector<cv::Rect> & windows)
  {
    coeffs.clear();
    if (l.coeffs_valid) coeffs.assign(l.coeffs, l.coeffs + 6);
    start.x = l.start_x;
    start.y = l.start_y;
    windows.clear();
    for (int i = 0; i < l.n_windows_up + l.n_windows_down; ++i) {
      cv::Rect w;
      w.x = l.windows[i][0];
      w.y = l.windows[i][1];
      w.width = l.windows[i][2];
      w.height = l.windows[i][3];
      windows.push_back(w);
    }
  }
  vp_lanes * lanes_ = nullptr;
  vp_lanes_result last_{};
};

}  // namespace autoware_pov::vision::egolanes

#endif  // LANE_FILTER_HIP_HPP_

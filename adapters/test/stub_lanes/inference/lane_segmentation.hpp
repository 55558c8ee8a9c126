// Compile-check stand-in for VisionPilot/production_release/include/inference/lane_segmentation.hpp:16-44, for lane_filter_check.cpp: the members
// EgoLanesHipEngine and LaneFilterHip fill, with the reference's names, types and defaults.  It is put ahead of test/stub on the include path; a real
// build includes the reference's own header.
#pragma once
#include <opencv2/opencv.hpp>

#include <vector>

namespace autoware_pov::vision::egolanes
{
struct LaneSegmentation
{
  cv::Mat ego_left, ego_right, other_lanes;
  int height = 0;
  int width = 0;
  std::vector<double> left_coeffs, right_coeffs;
  cv::Point left_start_point = {-1, -1};
  cv::Point right_start_point = {-1, -1};
  std::vector<cv::Rect> left_sliding_windows, right_sliding_windows;
};
}  // namespace autoware_pov::vision::egolanes

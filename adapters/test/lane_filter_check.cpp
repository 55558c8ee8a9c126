// Compile + behaviour check of adapters/lane_filter_hip.hpp (LaneFilterHip) and EgoLanesHipEngine::enqueue / handle against libvp_hip.so.
//   lane_filter_check                               -> the host fit and the null-handle conventions (no GPU needed)
//   lane_filter_check <blob> <frame.bgr> <h> <w> [fp32|fp16]
//       one packed BGR8 frame through engine.enqueue() + filter.update() as the production app's lateral thread would drive them, twice; the second
//       record of the same frame has the first one's device fields, and what update() returns is what the record holds
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "lane_filter_hip.hpp"

using autoware_pov::vision::egolanes::EgoLanesHipEngine;
using autoware_pov::vision::egolanes::LaneFilterHip;
using autoware_pov::vision::egolanes::LaneSegmentation;

static int fail(const char * what)
{
  std::fprintf(stderr, "lane_filter_check FAILED: %s\n", what);
  return 1;
}

// what LaneTracker::update reads of a LaneSegmentation: the members must exist with these types
static size_t consumed_like_the_tracker(const LaneSegmentation & s)
{
  const std::vector<double> & l = s.left_coeffs;
  const std::vector<double> & r = s.right_coeffs;
  const cv::Point a = s.left_start_point, b = s.right_start_point;
  const std::vector<cv::Rect> & wl = s.left_sliding_windows;
  const std::vector<cv::Rect> & wr = s.right_sliding_windows;
  return l.size() + r.size() + wl.size() + wr.size() + static_cast<size_t>(a.x + b.x + s.width + s.height);
}

int main(int argc, char ** argv)
{
  // --- host only: four points on the line x = y + 1, and the same four rows collapsed into one
  const int64_t S[5] = {4, 6, 14, 36, 98}, T[3] = {10, 20, 50}, S1[5] = {4, 8, 16, 32, 64};
  double abc[3] = {-1, -1, -1};
  int singular = -1;
  if (vp_lanes_fit(S, T, 1, abc, &singular) != VP_OK || singular != 0 || abc[0] != 0.0 || abc[1] != 1.0 || abc[2] != 1.0) return fail("vp_lanes_fit of a line");
  if (vp_lanes_fit(S1, T, 1, abc, &singular) != VP_OK || singular != 1 || abc[1] != 1.0) return fail("vp_lanes_fit must flag one row and leave out untouched");
  if (vp_lanes_fit(S, T, 3, abc, &singular) != VP_ERR_ARG || vp_lanes_fit(nullptr, T, 1, abc, &singular) != VP_ERR_ARG) return fail("vp_lanes_fit refusals");
  if (vp_lanes_pending(nullptr) != VP_ERR_ARG || vp_lanes_reset(nullptr) != VP_ERR_ARG) return fail("null handle");
  if (argc < 5) {
    std::puts("lane_filter_check: host conventions OK");
    return 0;
  }
  const std::string blob = argv[1], frame_path = argv[2], precision = argc > 5 ? argv[5] : "fp16";
  const int h = std::atoi(argv[3]), w = std::atoi(argv[4]);
  if (h < 1 || w < 1 || h > 16384 || w > 16384) return fail("frame geometry");
  std::vector<uint8_t> pixels((size_t)h * w * 3);
  std::ifstream ff(frame_path, std::ios::binary);
  ff.read(reinterpret_cast<char *>(pixels.data()), (std::streamsize)pixels.size());
  if (!ff) return fail("frame file too short");
  cv::Mat frame(h, w, CV_8UC3, pixels.data());

  EgoLanesHipEngine engine(blob, "hip", precision);
  LaneFilterHip filter(0.5f);
  if (engine.handle() == nullptr) return fail("handle()");
  if (filter.update(engine).width != 0) return fail("update before any pass must answer an empty LaneSegmentation");
  if (engine.enqueue(cv::Mat())) return fail("enqueue of an empty image must fail");
  const LaneSegmentation first = filter.update(frame, engine, 0.0f);
  if (first.width != 160 || first.height != 80 || !first.ego_left.empty()) return fail("update(): geometry, masks left empty");
  const vp_lanes_result r1 = filter.lastRecord();
  if (first.left_start_point.x != r1.lane[0].start_x || first.right_start_point.y != r1.lane[1].start_y) return fail("start points");
  if (first.left_sliding_windows.size() != (size_t)(r1.lane[0].n_windows_up + r1.lane[0].n_windows_down)) return fail("windows");
  if (first.left_coeffs.size() != (r1.lane[0].coeffs_valid ? 6u : 0u) || first.right_coeffs.size() != (r1.lane[1].coeffs_valid ? 6u : 0u)) return fail("coefficients");
  if (!engine.enqueue(frame)) return fail("enqueue");
  const LaneSegmentation second = filter.update(engine, 0.0f, true);
  const vp_lanes_result r2 = filter.lastRecord();
  if (second.ego_left.rows != 80 || second.ego_left.cols != 160) return fail("with_masks");
  for (int l = 0; l < 2; ++l)
    if (std::memcmp(&r1.lane[l], &r2.lane[l], offsetof(vp_lanes_lane, order)) != 0 || std::memcmp(r1.lane[l].raw_coeffs, r2.lane[l].raw_coeffs, sizeof(r1.lane[l].raw_coeffs)) != 0)
      return fail("the second record of the same frame differs from the first");
  filter.reset();
  std::printf("lane_filter_check: frame OK (%zu)\n", consumed_like_the_tracker(first) + consumed_like_the_tracker(second));
  return 0;
}

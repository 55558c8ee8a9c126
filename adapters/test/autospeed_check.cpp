// Compile + behaviour check of adapters/autospeed_hip_engine.hpp (AutoSpeedHipEngine) against libvp_hip.so.
//   autospeed_check                                     -> construction-failure conventions (no GPU needed)
//   autospeed_check <blob> <frame.bgr> <h> <w> <out> [fp32|fp16 [conf_thresh iou_thresh]]
//       one packed BGR8 frame through the engine as the production app's detector thread drives AutoSpeedOnnxEngine (inference(image, conf, iou));
//       writes to <out>: int32 n, n Detection records, int64 shape[3], the raw tensor [shape[1]][shape[2]] fp32
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "autospeed_hip_engine.hpp"

using autoware_pov::vision::autospeed::AutoSpeedHipEngine;
using autoware_pov::vision::autospeed::Detection;

static int fail(const char * what)
{
  std::fprintf(stderr, "autospeed_check FAILED: %s\n", what);
  return 1;
}

int main(int argc, char ** argv)
{
  // --- error conventions (the reference's ctor throws when the session cannot be built: onnxruntime_engine.cpp:13-66)
  try {
    AutoSpeedHipEngine e("/nonexistent/model.vpw");
    return fail("ctor with a missing weight file must throw");
  } catch (const std::runtime_error &) {
  }
  if (argc < 6) {
    std::puts("autospeed_check: construction-failure conventions OK");
    return 0;
  }
  const std::string blob = argv[1], frame_path = argv[2], out = argv[5], precision = argc > 6 ? argv[6] : "fp32";
  const int h = std::atoi(argv[3]), w = std::atoi(argv[4]);
  const float conf = argc > 8 ? (float)std::atof(argv[7]) : 0.25f, iou = argc > 8 ? (float)std::atof(argv[8]) : 0.45f;
  if (h < 1 || w < 1 || h > 16384 || w > 16384) return fail("frame geometry");
  std::vector<uint8_t> pixels((size_t)h * w * 3);
  std::ifstream ff(frame_path, std::ios::binary);
  ff.read(reinterpret_cast<char *>(pixels.data()), (std::streamsize)pixels.size());
  if (!ff) return fail("frame file too short");
  cv::Mat frame(h, w, CV_8UC3, pixels.data());

  AutoSpeedHipEngine e(blob, "hip", precision);
  if (e.getInputWidth() != 1024 || e.getInputHeight() != 512) return fail("model input size");
  try {
    e.getRawTensorData();
    return fail("getRawTensorData before inference must throw");
  } catch (const std::runtime_error &) {
  }
  try {
    e.getTensorShape();
    return fail("getTensorShape before inference must throw");
  } catch (const std::runtime_error &) {
  }
  cv::Mat bad(10, 10, CV_8UC1);
  try {
    e.inference(bad);
    return fail("a non-BGR8 image must throw");
  } catch (const std::runtime_error &) {
  }
  try {
    e.inference(cv::Mat());
    return fail("an empty image must throw");
  } catch (const std::runtime_error &) {
  }
  const std::vector<Detection> det = e.inference(frame, conf, iou);
  const std::vector<int64_t> shape = e.getTensorShape();
  if (shape.size() != 3 || shape[0] != 1 || shape[1] < 5 || shape[2] != 10752) return fail("tensor shape");
  std::ofstream f(out, std::ios::binary);
  const int n = (int)det.size();
  f.write(reinterpret_cast<const char *>(&n), sizeof n);
  f.write(reinterpret_cast<const char *>(det.data()), (std::streamsize)(det.size() * sizeof(Detection)));
  f.write(reinterpret_cast<const char *>(shape.data()), (std::streamsize)(3 * sizeof(int64_t)));
  f.write(reinterpret_cast<const char *>(e.getRawTensorData()), (std::streamsize)((size_t)shape[1] * shape[2] * sizeof(float)));
  // a second frame through the same object (the replayed graph): the same detections
  const std::vector<Detection> again = e.inference(frame, conf, iou);
  if (again.size() != det.size() || (n > 0 && std::memcmp(again.data(), det.data(), det.size() * sizeof(Detection)) != 0))
    return fail("the second inference() of the same frame differs from the first");
  // a threshold no score reaches: an empty vector, not an error
  if (!e.inference(frame, 2.0f, iou).empty()) return fail("conf_thresh above every score must give {}");
  if (!f) return fail("writing the output file");
  std::puts("autospeed_check: frame OK");
  return 0;
}

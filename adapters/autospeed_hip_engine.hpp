// AutoSpeedHipEngine -- drop-in for autoware_pov::vision::autospeed::AutoSpeedOnnxEngine / AutoSpeedTensorRTEngine
// (VisionPilot/middleware_recipes/common/backends/autospeed/onnxruntime_engine.hpp:26-132; implementation onnxruntime_engine.cpp:13-302),
// built on libvp_hip.so: a VP_AUTOSPEED engine (the detector network) attached to a vp_detect handle, one vp_detect_infer per frame --
// letterbox, network, decode + NMS on the device, one host synchronisation, no tensor in between on the host.  Same public methods and
// argument meaning, constructor arguments aside (the network's input is 512 x 1024: auto_speed_network.py:9-10).  Failure behaviour as
// AutoSpeedHipStages (autospeed_hip_stages.hpp): the ctor throws std::runtime_error; inference() throws on an image that is empty or not
// CV_8UC3 and on a DEVICE failure (VP_ERR_HIP), and returns {} with the reason on stderr for everything else (the reference returns {}
// when doInference fails, onnxruntime_engine.cpp:161-164); getRawTensorData() / getTensorShape() throw before the first inference (:288-302).
// Detection is the reference's struct; the detections are those of the two-call form on the engine's own tensor, bit for bit.
#ifndef AUTOSPEED_HIP_ENGINE_HPP_
#define AUTOSPEED_HIP_ENGINE_HPP_

#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include <opencv2/opencv.hpp>

#include "autospeed_hip_stages.hpp"  // Detection (detection.hpp:8-12 when the reference header is not on the include path)
#include "vp_hip.h"

namespace autoware_pov::vision::autospeed
{

class AutoSpeedHipEngine
{
public:
  // provider / cache_dir are accepted for signature compatibility (the ONNX / TensorRT engines use them); precision: "fp16" or "fp32"
  // (parity mode).  model_path: a VPW1 blob exported from the checkpoint (weights.py) or the detector's `.onnx` file.
  AutoSpeedHipEngine(const std::string & model_path, const std::string & provider = "hip", const std::string & precision = "fp16",
                     int device_id = 0, const std::string & cache_dir = "", bool latency_plan = false)
  {
    (void)provider;
    (void)cache_dir;
    char err[512] = {0};
    // the production app runs this engine on its own thread beside EgoLanes / AutoSteer on the same GPU (production_release/main.cpp:505-535):
    // the default kernel plan; latency_plan = true is for a host that runs it alone
    const int prec = ((precision == "fp32" || precision == "fp16x3") ? VP_FP16X3 : VP_FP16) | (latency_plan ? VP_PLAN_LATENCY : 0);
    if (vp_create(&engine_, VP_AUTOSPEED, model_path.c_str(), prec, device_id, err, sizeof(err)) != VP_OK)
      throw std::runtime_error(std::string("[hip_engine] ") + err);
    vp_input_hw(engine_, &in_h_, &in_w_);
    // vp_output_shape answers only after a pass: the handle is sized for up to 80 classes, vp_detect_attach refuses a wider head
    if (vp_detect_create(&detect_, device_id, in_h_, in_w_, kPredictions, kMaxChannels, err, sizeof(err)) != VP_OK) {
      vp_destroy(engine_);
      throw std::runtime_error(std::string("[hip_engine] ") + err);
    }
    if (vp_detect_attach(detect_, engine_) != VP_OK) {
      const std::string msg = std::string("[hip_engine] ") + vp_detect_last_error(detect_);
      vp_detect_destroy(detect_);
      vp_destroy(engine_);
      throw std::runtime_error(msg);
    }
    out_.resize(static_cast<size_t>(kPredictions));
  }
  ~AutoSpeedHipEngine()
  {
    vp_detect_destroy(detect_);  // the handle borrows the engine: it goes first
    vp_destroy(engine_);
  }
  AutoSpeedHipEngine(const AutoSpeedHipEngine &) = delete;
  AutoSpeedHipEngine & operator=(const AutoSpeedHipEngine &) = delete;

  unsigned long long planHash() const { return vp_plan_hash(engine_); }

  // AutoSpeedOnnxEngine::inference (onnxruntime_engine.cpp:154-168): detections in the coordinates of input_image
  std::vector<Detection> inference(const cv::Mat & input_image, float conf_thresh = 0.25f, float iou_thresh = 0.45f)
  {
    if (input_image.empty() || input_image.type() != CV_8UC3)   // the C call is never made: its last-error text would be a stale one
      throw std::runtime_error("[hip_engine] inference: input image is empty or not CV_8UC3");
    int n = 0;
    const int rc = vp_detect_infer(detect_, input_image.data, input_image.rows, input_image.cols, static_cast<int>(input_image.step), conf_thresh,
                                   iou_thresh, reinterpret_cast<vp_detection *>(out_.data()), static_cast<int>(out_.size()), &n);
    if (rc == VP_ERR_HIP) throw std::runtime_error(std::string("[hip_engine] inference: ") + vp_detect_last_error(detect_));
    if (rc != VP_OK) {
      std::fprintf(stderr, "[hip_engine] inference: %s\n", vp_detect_last_error(detect_));
      return {};
    }
    ran_ = true;
    return std::vector<Detection>(out_.begin(), out_.begin() + n);
  }

  // the network's output tensor of the last inference(), fp32 [4 + nc][10752] on the host (fetched from the device on the first call per frame)
  const float * getRawTensorData() const
  {
    const float * raw = nullptr;
    int64_t shape[4];
    if (!ran_ || vp_logits(engine_, &raw, shape) != VP_OK)
      throw std::runtime_error("Inference has not been run yet. Call inference() first.");
    return raw;
  }
  // [batch, 4 + nc, predictions], the shape the reference's engines report for the same tensor
  std::vector<int64_t> getTensorShape() const
  {
    int64_t shape[4];
    if (!ran_ || vp_output_shape(engine_, shape) != VP_OK)
      throw std::runtime_error("Inference has not been run yet. Call inference() first.");
    return {shape[0], shape[1], shape[3]};
  }
  int getInputWidth() const { return in_w_; }
  int getInputHeight() const { return in_h_; }
  const char * lastError() const { return vp_detect_last_error(detect_); }

private:
  static constexpr int kPredictions = 10752;  // 64 x 128 + 32 x 64 + 16 x 32 anchors of the 512 x 1024 input
  static constexpr int kMaxChannels = 4 + 80; // 4 box rows + up to 80 classes
  vp_engine * engine_ = nullptr;
  vp_detect * detect_ = nullptr;
  int in_h_ = 0, in_w_ = 0;
  bool ran_ = false;
  std::vector<Detection> out_;
};

}  // namespace autoware_pov::vision::autospeed

#endif  // AUTOSPEED_HIP_ENGINE_HPP_

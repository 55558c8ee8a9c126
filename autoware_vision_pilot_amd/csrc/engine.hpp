// Host-side engine of libvp_hip: weight blob -> folded/packed device weights -> static per-model launch plan
// (one HIP stream, replayed as a hipGraph) behind the C ABI of include/vp_hip.h.
#pragma once
#include <cmath>
#include <functional>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "kernels.hpp"

namespace vp {

struct HostTensor {
  std::vector<int> shape;
  std::vector<float> data;
  size_t numel() const { return data.size(); }
};

// "VPW1" container: u32 count, then per tensor {u16 name_len, name, u8 ndim, u32 dims[ndim], fp32 data}.
// Written by autoware_vision_pilot_amd/weights.py from a reference state_dict (keys kept verbatim).
class WeightBlob {
 public:
  void parse(const void* blob, size_t bytes);
  const HostTensor& get(const std::string& key) const;
  bool has(const std::string& key) const { return t_.count(key) != 0; }
  size_t size() const { return t_.size(); }
  // FNV-1a over (key suffix, shape, fp32 bytes) of every tensor whose key starts with `prefix`, in key order:
  // equal hashes <=> the sub-network under that prefix carries the same parameters (shared-prefix engines).
  unsigned long long group_hash(const std::string& prefix) const;
  // BASELINE configs[4] "fp8 weights": every conv / linear weight -> per-output-channel symmetric OCP e4m3 (max 448,
  // 3 mantissa bits, subnormals), stored back DE-quantised (oracle/autodrive.py quantize_fp8_e4m3, same arithmetic).
  void quantize_fp8_e4m3();

 private:
  std::map<std::string, HostTensor> t_;
};

// onnx_reader.cpp: ONNX file (reference exporter settings) -> tensors in state_dict naming / the same as a VPW1 blob.
std::map<std::string, HostTensor> load_onnx_state_dict(const std::string& path);
std::vector<char> onnx_to_blob(const std::string& path);

// Pillow's resample coefficient tables (engine.cpp): bounds [out][2], coefficients [out][ksize] with 22 fractional bits; returns ksize
int pil_coeffs(int in_size, int out_size, int filter, std::vector<int>* bounds, std::vector<int>* kk);
// 11-bit fixed-point bilinear taps of the cv::resize INTER_LINEAR restatement ([dst][4] = i0, i1, w0, w1; engine_io.cpp, oracle/pre_post.py linear_taps_u8)
void linear_taps_u8(int src, int dst, std::vector<int>* tab);

// a value left the representable range (vp_status VP_ERR_RANGE): a weight beyond fp16 at load, inf / NaN in a network's output
struct RangeError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

struct Act {
  std::string name;
  int Creal = 0, C = 0, H = 0, W = 0;
  int frames = 1;  // batched encoder: `frames` camera frames stacked along H (H = frames * per-frame height)
  half_t* hi = nullptr;
  half_t* lo = nullptr;
  int tie = -1;    // VP_ACT_SCALE engines: index of the exponent this tensor is stored with (Engine::act_exp_); tensors that share storage or a copy share it
  ActView view() const { return ActView{hi, lo, H, W, C}; }
  size_t elems() const { return (size_t)H * W * C; }
};

struct Op {
  std::string name;
  std::string kernel;  // kernel instantiation tag (groups launches for the roofline report)
  std::string launch;  // launch geometry fixed at PLAN time that the tag does not spell (split-K factor, persistent-group count): hashed by vp_plan_hash
  double flops = 0, bytes = 0;
  // matrix work the launch EXECUTES when that differs from the reference formulation's count in `flops` (composed up-sampling stages: flops keeps
  // SURVEY.md 8d's three-op count so whole-frame figures stay comparable across rounds); 0 = same as flops
  double flops_executed = 0;
  std::function<hipError_t(hipStream_t)> run;
  std::vector<const Act*> writes;  // the tensors this launch stores in HBM: what vp_calibrate_range and vp_range_survey measure behind it (host bookkeeping only)
};

// ConvTranspose2d(k2, s2) [+ 1x1 skip link] -> Conv3x3 multiplied out at load (engine_upconv.cpp): fp64, real (un-padded) channel counts
struct UpconvComposed {
  int cin = 0, cm = 0, cout = 0, cs = 0;
  std::vector<double> wx;    // [4 phases (py * 2 + px)][4 taps (a * 2 + b)][cout][cin]: out(2y + py, 2x + px) += wx . x(y + py - 1 + a, x + px - 1 + b)
  std::vector<double> ws;    // [9 taps (ty * 3 + tx)][cout][cs]: 3x3 convolution of the skip tensor
  std::vector<double> bias;  // [9 classes (row class * 3 + column class)][cout]; class 0 / 1 / 2 = first / inner / last row (column) of the output map
};

struct ConvOpts {
  int act = ACT_NONE;
  int res_mode = RES_NONE;
  const Act* res = nullptr;
  int tile = -1, bk = -1, nsplit = -1;
  float* logits_out = nullptr;  // STORE_NCHW_F32 target
  const Act* in2 = nullptr;     // K-extension tensor of the fused ConvTranspose + skip-link GEMM (add_convT_skip)
  int stride = 1;               // 3x3 stride-2 convs of AutoDrive (generic GEMM kernel only)
  int post_act = ACT_NONE;      // activation after the residual (CTX: SiLU(c4*x + x))
  bool pixel_shuffle = false;   // set by add_convT*: the GEMM stores with STORE_SHUFFLE2 (never the pointwise kernel)
};

// Frame pools registered for DMA (vp_register_frames): process-wide, engine_io.cpp
int register_frame_range(const void* pool, size_t bytes);
int unregister_frame_range(const void* pool);
bool frame_range_registered(const void* p, size_t bytes);

// What a consumer sees of a device-resident camera frame (vp_frame, vp_handle.hpp): packed BGR8 rows `pitch` bytes apart on GPU `gpu`, complete on the
// device once `ready` has fired.  bgr == nullptr: nothing was uploaded yet.
struct FrameView {
  const uint8_t* bgr = nullptr;
  int h = 0, w = 0, pitch = 0, gpu = 0;
  hipEvent_t ready = nullptr;
};
// the region (x0, y0, w, h) of a frame as a consumer takes it (w == h == 0: the whole frame); throws std::invalid_argument / std::runtime_error
void resolve_frame_region(const FrameView& f, int x0, int y0, int* w, int* h);

// Where an engine's resident input came from (vp_canvas draws there): the region (x0, y0, w, h) of a source frame of H x W.  vp_upload_from_frame /
// vp_infer_frame record the region they took; the host uploads record the whole frame, (0, 0, w, h) of h x w.  H == 0: no frame was taken yet.
struct SourceRegion {
  int x0 = 0, y0 = 0, w = 0, h = 0, H = 0, W = 0;
};

struct ConvChoice;   // engine_internal.hpp: what the dispatch rules of engine_dispatch.cpp give one convolution
struct HostWeights;  // engine_internal.hpp: a layer's packed weights on the host

class Engine {
 public:
  // base != nullptr builds a SHARED-PREFIX engine (vp_create_shared): sub-networks whose parameters equal the base
  // engine's (backbone; backbone + context + neck) are not rebuilt -- this engine's plan starts from the base
  // engine's feature tensors and runs on the base engine's stream, after it, on the frame the base last processed.
  // frames > 1 (base == nullptr): BATCHED ENCODER -- preprocess + EfficientNet backbone of `frames` camera frames per pass,
  // no context / neck / head; its taps feed shared-prefix engines built with (base = this, frame_index = f).
  Engine(int kind, const WeightBlob* blob, int precision, int gpu_id, Engine* base = nullptr, int frames = 1, int frame_index = 0);
  ~Engine();
  Engine(const Engine&) = delete;
  Engine& operator=(const Engine&) = delete;

  // configuration
  void set_input_format(int pixel_format, int plane_order);
  void set_decode_mode(int mode);
  // u8 -> [0, 1] ahead of (x - mean) / std: 0 = q / 255 (torchvision to_tensor: the Python operator API), 1 = q * fl(1/255)
  // (cv::Mat::convertTo(CV_32FC3, 1.0 / 255.0): the C++ front-ends, onnx_runtime_backend.cpp:45, onnxruntime_engine.cpp:85)
  void set_norm_form(int form);
  int norm_form() const { return norm_form_; }
  // AutoSteer hand-over: the raw EgoLanes logits of the last TWO passes, [t-1 | t] = fp32 {1, 6, 80, 160}, kept on the device and
  // updated behind every pass (production_release main.cpp:472-534 builds the same buffer on the host with a circular buffer and two memcpys)
  void set_lane_ring(bool on);
  bool lane_ring() const { return lane_ring_; }
  float* dev_lane_ring() const { return d_lane_ring_; }
  int lane_ring_frames() const { return ring_frames_; }   // 0, 1, 2: the reference runs AutoSteer only once two frames are in
  void fetch_lane_ring(float* dst);                        // D2H of the 6 x 80 x 160 floats + sync
  // frame resize ahead of the network: 0 = the integer bilinear modelled on cv::resize INTER_LINEAR (the C++ nodes; default of the scene
  // networks), 1 / 2 = Pillow's antialiased BILINEAR / BICUBIC (the Python scripts' Image.resize; 1 is AutoDrive's default)
  void set_resize_mode(int mode);
  int resize_mode() const { return resize_mode_; }
  int net_h() const { return kind_ >= 4 && kind_ <= 6 ? 512 : 320; }   // AutoDrive: autodrive_network.py:8-9, AutoSpeed: auto_speed_network.py:9-10, AutoSteer: auto_steer_network.py:9-10
  int net_w() const { return kind_ >= 4 && kind_ <= 6 ? 1024 : 640; }
  int kind() const { return kind_; }
  // AutoSpeed (kind 5): the network input on the device ([3][512][1024] fp32 planes R, G, B in [0, 1]) for a producer on the same GPU (vp_detect_infer's
  // letterbox kernel writes it), and the note that it now holds this frame's tensor
  float* dev_input() const { return d_input_; }
  void note_device_tensor();
  // AutoDrive (kind 4) pairs every frame with the previous one: infer_pair() runs the backbone on `prev` first
  // (features only), enqueue() then shifts the feature slots and runs backbone + head on the resident frame.
  void prime_previous();

  // frame path
  void upload_frame(const uint8_t* frame, int h, int w, int stride, int index = 0);  // index: slot of a batched encoder
  // the asynchronous twin for a device-resident camera frame (vp_frame): this engine's stream waits for the frame's content, then copies the region
  // (x0, y0, w, h; w == h == 0: the whole frame) device to device into the engine's own frame buffer, rows packed.  The caller records the "consumer
  // done" event behind it (vp_api.cpp).
  void upload_from_frame(const FrameView& f, int x0, int y0, int w, int h);
  int frames() const { return frames_; }
  void upload_tensor(const float* nchw);
  void enqueue();
  void sync();
  void fetch_outputs();      // enqueue_fetch() + sync
  void enqueue_fetch();      // async D2H of the selected outputs (set_outputs) into the pinned host buffers
  void enqueue_status_fetch();  // async D2H of the range probe's verdict only
  // bit 0: logits, bit 1: mask.  De-selected outputs stay in HBM and are copied on first use (vp_logits / vp_mask_u8).
  void set_outputs(int mask) {
    if (mask < 0 || mask > 3) throw std::invalid_argument("outputs: bit 0 = logits, bit 1 = mask");
    outputs_ = mask;
  }
  // stage vp_infer's H2D through a pinned double buffer owned by the engine (default on)
  void set_pinned_staging(bool on) { pinned_staging_ = on; }
  // inf / NaN probe on the logits at the end of every pass (default on; a 3 us kernel): reported by the next synchronising call
  void set_finite_check(bool on) {
    if (on != finite_check_) {
      finite_check_ = on;
      graph_valid_ = false;
      ++plan_epoch_;
    }
  }
  void check_status();  // throws RangeError if the last fetched pass flagged a non-finite output
  bool poll_status();   // the same verdict without the throw (vp_infer_multi polls every member, then reports once)
  void copy_outputs_device(void* logits_dst, void* mask_dst);
  void mask_resized(uint8_t* dst, int h, int w);
  void depth_resized(float* dst, int h, int w);
  void visualize_mask(int viz_type, uint8_t* dst_bgr, int dst_h, int dst_w);
  void visualize_depth(uint8_t* dst_bgr, int h, int w);
  void read_input_tensor(float* dst);

  const float* host_logits();   // pinned host copy; fetched now if the last pass did not copy it
  const uint8_t* host_mask();
  int frame_h() const { return frame_h_; }
  int frame_w() const { return frame_w_; }
  const SourceRegion& source_region() const { return base_ ? base_->source_region() : src_region_; }   // a shared-prefix head: its base's
  void* dev_logits() const { return d_logits_; }
  void* dev_mask() const { return d_mask_; }
  float* alloc_f32(size_t n) { return static_cast<float*>(dalloc(n * sizeof(float))); }  // test operator entry: a logits buffer
  int out_c() const { return out_c_; }
  int out_h() const { return out_h_; }
  int out_w() const { return out_w_; }
  bool have_outputs() const { return have_outputs_; }
  void use_graph(bool on) { use_graph_ = on; }

  void timer_begin();
  float timer_end();
  int profile_layers(int iters, float* ms, int cap);

  const std::vector<Op>& ops() const { return ops_; }
  const std::vector<std::unique_ptr<Act>>& acts() const { return acts_; }
  void read_act(int i, float* dst);

  // plan-building blocks (public for the single-op test entry)
  Act* new_act(const std::string& name, int creal, int h, int w);
  Act* add_conv(const std::string& name, const Act* in, const std::vector<float>& w, const std::vector<float>& b, int cout, int ks,
                const ConvOpts& o, Act* out_override = nullptr);
  Act* add_convT_skip(const std::string& up_name, const std::string& skip_name, const Act* in, const Act* skip_in,
                      const std::vector<float>& wt, const std::vector<float>& bt, const std::vector<float>& ws,
                      const std::vector<float>& bs, int cout);
  Act* add_convT(const std::string& name, const Act* in, const std::vector<float>& w, const std::vector<float>& b, int cout,
                 const ConvOpts& o);
  void compose_upconv(const float* wt, const float* bt, const float* ws, const float* bs, const float* w3, const float* b3, int cin, int cm, int cout,
                      int cs, UpconvComposed* out);
  // shape: 6 / 7 (kernels.hpp), -1 = dispatch rule; nsplit: K slices, <= 0 = dispatch rule
  Act* add_upconv(const std::string& name, const Act* in, const Act* skip_in, const std::vector<float>& wt, const std::vector<float>& bt,
                  const std::vector<float>& ws, const std::vector<float>& bs, const std::vector<float>& w3, const std::vector<float>& b3, int cm,
                  int cout, int act, int shape = -1, int nsplit = 0, const std::string& out_name = std::string());
  bool upconv_wanted() const;  // composed up-sampling stages in this engine's plan (parity mode; VP_UPCONV=0: the three-op form of rounds 1-5)
  Act* alias_slice(const std::string& name, Act* whole, int ch_off, int nch);  // view of channels [ch_off, ch_off + nch) with the tensor's row pitch (no allocation)
  void run_eager();
  void run_ops(hipStream_t st, size_t begin, size_t end);
  void enqueue_multi(const std::vector<Engine*>& heads);
  void set_multi_fork(bool on) { multi_fork_ = on; }
  void upload_act(Act* a, const float* chw);
  hipStream_t stream() const { return stream_; }
  int gpu() const { return gpu_; }
  int decode_mode() const { return decode_mode_; }
  bool host_logits_current() const { return host_logits_valid_; }  // the pinned host logits belong to the LAST pass
  bool split() const { return (precision_ & 15) == 1; }
  bool fp8_weights() const { return (precision_ & 16) != 0; }
  // VP_ACT_SCALE (creation flag, AutoDrive / AutoSpeed / AutoSteer in the parity mode and the operator entries): every activation tensor t is stored as x * 2^-s_t
  bool act_scale() const { return (precision_ & 64) != 0; }
  int act_exp(const Act* a) const { return (a && a->tie >= 0) ? act_exp_[a->tie] : 0; }
  float act_mul(const Act* a, int sign = 1) const { return std::ldexp(1.0f, sign * act_exp(a)); }   // 2^(sign * s_a)
  void tie_acts(const Act* a, const Act* b);   // plan time: b's tensors take a's exponent (copies, max-pools, alias slices: s_out == s_in)
  void set_act_exp(const Act* a, int e);       // operator entry / tests
  // operator entry / tests: cat([up(a), b]) the way the necks build it, the tie of a, b and out included
  void add_up_cat(const std::string& name, const Act* a, const Act* b, Act* out, int a_off, int a_nch, int b_off, int b_nch) {
    neck_up_cat(name, a, b, out, a_off, a_nch, b_off, b_nch);
  }
  void calibrate_range(int target_log2);
  // vp_range_survey (include/vp_hip.h): one entry per acts() entry, count == 0 where the plan never stores the tensor
  struct RangeStats {
    float absmax = 0.0f;
    int exp = 0;
    unsigned long long count = 0, nonfinite = 0, zeros = 0, bins[VP_HIST_BINS] = {};
  };
  std::vector<RangeStats> range_survey();
  void reset_range();
  std::vector<int> act_scales() const;                  // one per acts() entry
  void set_act_scales(const int* exps, int n);
  // VP_MFMA_FP8 (creation flag, VP_FP16 scene networks that own their whole network, and the operator entry): the plain big 3x3 layers run on the e4m3
  // MFMA kernel; every such layer quantises its input as e4m3(x * 2^-qexp) with a per-layer exponent (include/vp_hip.h "FP8 MFMA ENGINES")
  bool mfma_fp8() const { return (precision_ & 128) != 0; }
  struct Fp8Layer {
    size_t op = 0;     // launch index (ops())
    int tensor = -1;   // the input tensor's index in acts()
    int qexp = 0;
    bool seen = false; // measured or installed since the last reset: a later calibration only raises it
  };
  const std::vector<Fp8Layer>& fp8_layers() const { return f8_layers_; }
  void calibrate_fp8(int target_log2);
  void reset_fp8();
  void set_fp8_exps(const int* exps, int n);
  void stash_previous_frame();                          // AutoDrive: keeps the frame vp_infer_pair primes with, so that a calibration can run the pair again
  // kernel plan target of THIS engine (round 6: a creation flag, VP_PLAN_LATENCY; the process-wide developer option VP_PLAN_TARGET still selects it for
  // every engine created while it is set): the round-4 choices for the CU-time rules of engine_dispatch.cpp
  bool plan_latency() const;
  // ... kept as e4m3 BYTES in HBM (round 4): AutoDrive engines (BASELINE configs[4]) and the operator entry; a scene network with the flag keeps
  // de-quantised fp16 planes on its LDS-DMA / register-stationary kernels
  bool fp8_storage() const { return fp8_weights() && (kind_ == 4 || kind_ < 0); }
  int shared_level() const { return shared_level_; }  // 0 own network, 1 backbone shared, 2 backbone + context + neck shared
  // device bytes of the network's WEIGHT tensors by storage class (bias / scale vectors and tables not counted): [0] e4m3 codes, [1] fp16 planes, [2] fp32
  const unsigned long long* weight_bytes() const { return wbytes_; }

  std::string last_error;

 private:
  struct PackedConv {
    half_t* w_hi = nullptr;
    half_t* w_lo = nullptr;
    float* bias = nullptr;
    float* wscale = nullptr;  // [CoutW] 2^-prescale of the weight rows (engine_internal.hpp prescale_exp), or the fp8 row scales
    uint8_t* w8 = nullptr;    // VP_WEIGHTS_FP8 on a kernel that stages weights through registers: e4m3 codes in that kernel's layout (w_hi / w_lo null)
    int CoutW = 0, tile = 0, bk = 32, nsplit = 1;
    PackedConv() = default;
    explicit PackedConv(const ConvChoice& c);
  };
  void construct(int kind, const WeightBlob* blob, int precision, int gpu_id, Engine* base);
  void release();  // frees every device / host resource; idempotent (destructor and failed construction)
  void* dalloc(size_t bytes, bool zero = true);
  void dfree(void* p);  // hipFree + forget (buffers that are re-grown at run time; the caller has synchronised the stream)
  // Synchronous copies / fills WITHOUT the legacy stream: hipMemcpy / hipMemset run on the NULL stream, which implicitly joins every blocking
  // stream of the device, and the runtime refuses that while ANY thread captures a graph ("would make the legacy stream depend on a
  // capturing ... stream") -- an engine created or read on one host thread invalidated the capture another thread's engine was recording
  // (round 4: seen once vp_create got fast enough to overlap it).  These go through the engine's own non-blocking stream and wait for it.
 public:
  void copy_h2d(void* d, const void* h, size_t bytes);
  void copy_d2h(void* h, const void* d, size_t bytes);
  void fill_zero(void* d, size_t bytes);
 private:
  template <class T>
  void upload_grow(T*& d, size_t& cap_elems, const std::vector<T>& v);  // re-uses d while v fits, else frees it and allocates anew
  const void* zero_page();  // 256 bytes of zeros in device memory (LDS-DMA source for out-of-image pixels, kernels_head.hip)
  template <class T>
  T* dupload(const std::vector<T>& v);
  // FC matrix [N][K] -> fp32 rows, or (VP_WEIGHTS_FP8) e4m3 codes + row scales.  row_amax: per-row maximum the quantiser saw when it is not the
  // maximum of the K values handed in (AutoDrive's exp0: a row's three Conv1d taps share one scale, only the centre tap is used), else null
  void upload_fc_weights(FcParams* fp, const std::vector<float>& w, int N, int K, const std::vector<float>* row_amax = nullptr);
  void upload_packed(PackedConv* pc, const HostWeights& hw);  // hi, lo | codes, then bias, then the row scales
  void push_conv_op(const std::string& name, const Act* in, const PackedConv& pc, int ks, int ncols, const ConvOpts& o, Act* out,
                    int store_mode, int cout_real);

  void build_model(const WeightBlob& blob);
  void build_autodrive(const WeightBlob& blob);
  void build_autospeed(const WeightBlob& blob);
  void build_autosteer(const WeightBlob& blob);
  // the backbone AutoDrive, AutoSpeed and AutoSteer share (engine.cpp): P2 / P3 / P4 / P5 and the index of the launch that stores P5
  struct AdFeatures {
    Act* p2 = nullptr;
    Act* p3 = nullptr;
    Act* p4 = nullptr;
    Act* p5 = nullptr;
    size_t p5_op = 0;
  };
  AdFeatures build_ad_backbone(const WeightBlob& blob, const std::string& prefix, const std::function<Act*(int, int, int)>& p5_dest);
  void push_op(const std::string& name, const char* kernel, std::function<hipError_t(hipStream_t)> fn, double flops = 0, double bytes = 0);
  // blocks of the AutoSpeed / AutoSteer necks (engine.cpp, in front of build_autospeed): Conv + BN + SiLU [+ residual behind the activation], a channel
  // slice copy, C3K2 (common_layers.py:166-180) and cat([up(a), b]) as one launch
  Act* neck_conv_bn(const WeightBlob& blob, const std::string& name, const Act* in, int ks, int stride, const Act* res = nullptr, Act* dst = nullptr);
  void neck_copy_slice(const std::string& name, const Act* src, int src_off, const Act* dst, int dst_off, int nch);
  Act* neck_c3k2(const WeightBlob& blob, const std::string& p, const Act* in, bool csp, Act* dst);
  // channels [a_off, a_off + a_nch) of a and [b_off, b_off + b_nch) of b; a_nch / b_nch 0 = the whole tensor
  void neck_up_cat(const std::string& name, const Act* a, const Act* b, Act* out, int a_off = 0, int a_nch = 0, int b_off = 0, int b_nch = 0);
  std::vector<Act*> build_backbone(const WeightBlob& blob, const std::string& prefix);
  Act* build_context(const WeightBlob& blob, const std::string& p, const Act* deep, int cctx);
  Act* build_neck(const WeightBlob& blob, const std::string& p, const Act* ctx, const std::vector<Act*>& feats, int cctx);
  void build_head(const WeightBlob& blob, const std::string& p, const Act* neck, const std::vector<Act*>& feats);
  void finish_plan();
  void ensure_tables(int h, int w);
  // the two halves of a frame upload: "accept this geometry" (refusals, buffer, tap tables, graph invalidation; returns where the bytes go) and, behind
  // the copy each path queues itself, "a frame is the input now"
  void refuse_frame_input() const;
  uint8_t* accept_frame_geometry(bool have_bytes, int h, int w, int stride, int index);
  void note_frame_input();
  void capture_graph();

  Act* frame_view(const Act* a, int f);  // per-frame window of a stacked activation (no allocation)
  int kind_, precision_, gpu_;
  int wlo_keep_ = 10;  // experiment knob VP_WLO_KEEP_BITS, read once in construct(): mantissa bits this engine's low weight planes keep (10 = all)
  int frames_ = 1, frame_index_ = 0;
  hipStream_t stream_ = nullptr;
  Engine* base_ = nullptr;
  int shared_level_ = 0;
  unsigned long long hash_bb_ = 0, hash_ctx_ = 0, hash_neck_ = 0;
  std::vector<Act*> feats_;   // backbone taps f0..f4 (kept for shared-prefix engines)
  Act* neck_out_ = nullptr;
  std::vector<int> act_exp_;        // VP_ACT_SCALE: exponent per tie group (Act::tie)
  std::vector<char> act_exp_seen_;  // ... measured since the last reset: a later measurement only raises it
  std::vector<Fp8Layer> f8_layers_; // VP_MFMA_FP8: one per conv3x3_f8 launch, in launch order (the launches read qexp when they run)
  unsigned* d_absmax_ = nullptr;
  unsigned long long* d_survey_ = nullptr;   // range_survey: per tensor {abs-max bits | non-finite count << 32 as two words, VP_HIST_WORDS counters}
  // The eager launch-by-launch walk calibrate_range and range_survey share (engine_io.cpp): visit(i, a, begin, prime) runs behind launch i for every
  // tensor a it stores; `begin` is the first launch of the pass, `prime` marks AutoDrive's features-only pass over the previous frame.  visit returns
  // false to start the round over; walk_stored returns whether a round ran to its end.
  using StoredVisitor = std::function<bool(size_t i, const Act* a, size_t begin, bool prime)>;
  bool walk_stored(const StoredVisitor& visit);
  uint8_t* d_prev_frame_ = nullptr;
  size_t prev_frame_cap_ = 0;
  bool prev_frame_stashed_ = false;  // stash_previous_frame() ran and no frame was uploaded since
  bool prev_frame_valid_ = false;    // the stash is the frame the pair's previous half came from: true only while the upload right behind the stash is the resident frame
  void exps_changed() { graph_valid_ = false; ++plan_epoch_; }
  size_t ad_shift_op_ = 0, ad_place_op_ = 0;  // AutoDrive: ops_[shift] moves curr->prev features, ops_[place] stores the new ones
  bool ad_primed_ = false;
  std::vector<void*> allocs_;
  unsigned long long wbytes_[3] = {0, 0, 0};
  std::vector<std::unique_ptr<Act>> acts_;
  std::vector<Op> ops_;
  size_t first_net_op_ = 0;  // ops_[0] is the preprocess op (skipped for vp_infer_tensor)

  // input
  int pixel_format_ = 0, plane_order_ = 0, decode_mode_ = 0, norm_form_ = 0;
  uint8_t* d_frame_ = nullptr;
  size_t frame_cap_ = 0;
  int frame_h_ = 0, frame_w_ = 0, frame_stride_ = 0;
  SourceRegion src_region_;
  friend class Canvas;   // reads the last mask / logits on the device and orders its stream against this engine's
  friend class Metric;   // reads the last logits on the device, ordered the same way
  friend class Lanes;    // the same
  int* d_xtab_ = nullptr;
  int* d_ytab_ = nullptr;
  int tab_h_ = 0, tab_w_ = 0;
  float* d_input_ = nullptr;  // [3][320][640]
  int resize_mode_ = 0;
  int* d_pil_hb_ = nullptr;
  int* d_pil_hk_ = nullptr;
  int* d_pil_vb_ = nullptr;
  int* d_pil_vk_ = nullptr;
  int pil_hks_ = 0, pil_vks_ = 0;
  size_t pil_cap_[5] = {0, 0, 0, 0, 0};  // capacities (elements) of hb, hk, vb, vk, tmp
  uint8_t* d_pil_tmp_ = nullptr;
  PilResampleParams pil_params(const PreprocessParams& pp) const;
  bool input_is_tensor_ = false;

  // outputs
  int out_c_ = 0, out_h_ = 0, out_w_ = 0;
  float* d_logits_ = nullptr;
  uint8_t* d_mask_ = nullptr;
  void* d_zero_ = nullptr;
  float* h_logits_ = nullptr;
  uint8_t* h_mask_ = nullptr;
  bool have_outputs_ = false;
  bool decode_fused_ = false;  // the logits convolution writes d_mask_ in its epilogue: no separate decode launch
  int outputs_ = 3;  // vp_set_outputs: bit 0 logits, bit 1 mask copied to the host by vp_infer*
  bool host_logits_valid_ = false, host_mask_valid_ = false;
  float* d_lane_ring_ = nullptr;  // [6][out_h][out_w] fp32: previous | current EgoLanes logits (vp_set_lane_ring)
  bool lane_ring_ = false;
  int ring_frames_ = 0;
  void note_pass() { if (lane_ring_ && ring_frames_ < 2) ++ring_frames_; }
  unsigned* d_status_ = nullptr;  // sticky non-finite flag written by the probe kernel
  unsigned* h_status_ = nullptr;  // pinned copy, fetched with the outputs
  bool finite_check_ = true, status_pending_ = false;
  // pinned staging of the caller's (pageable) frame: two slots
  uint8_t* h_frame_ = nullptr;
  size_t h_frame_cap_ = 0;
  int h_frame_slot_ = 0;
  hipEvent_t h_frame_ev_[2] = {nullptr, nullptr};  // recorded behind the H2D that reads a slot; awaited before the slot is rewritten
  bool pinned_staging_ = true;

  // split-K scratch
  std::vector<float**> partial_slots_;

  // resize scratch
  void* d_resize_out_ = nullptr;
  size_t resize_cap_ = 0;
  int* d_rs_tab_ = nullptr;
  uint8_t* d_viz_lut_ = nullptr;  // [3 viz types][256][3]
  uint8_t* d_viridis_ = nullptr;  // [256][3] BGR (viridis_lut.inc)
  unsigned* d_minmax_ = nullptr;  // order keys of the depth plane's min / max
  void* d_depth_viz_ = nullptr;
  size_t depth_viz_cap_ = 0;
  void resize_depth_on_device(int h, int w);  // fp32 h x w plane -> d_resize_out_
  std::vector<int> rs_idx_host_;
  std::vector<float> rs_wgt_host_;
  size_t rs_tab_cap_ = 0;

  // graph
  bool use_graph_ = true;
  hipGraph_t graph_ = nullptr;
  hipGraphExec_t graph_exec_ = nullptr;
  // enqueue_multi: ONE graph for this engine and its shared-prefix heads, the heads that need only the backbone forked onto side
  // streams behind it (they overlap this engine's own context / neck / head); keyed by the head list and every member's plan epoch
  hipGraph_t multi_graph_ = nullptr;
  hipGraphExec_t multi_exec_ = nullptr;
  std::vector<std::pair<const Engine*, unsigned long long>> multi_key_;
  std::vector<hipStream_t> side_streams_;
  std::vector<hipEvent_t> side_events_;   // [0] fork, [1 + i] join of side stream i
  bool multi_fork_ = true;                // vp_set_multi_fork
  size_t n_fork_ops_ = 0;                 // ops_[0, n_fork_ops_): preprocess + backbone (what a level-1 head consumes)
  unsigned long long plan_epoch_ = 0;     // bumped whenever graph_valid_ is cleared
  bool graph_valid_ = false;
  bool warmed_ = false;
  hipEvent_t ev0_ = nullptr, ev1_ = nullptr;
};

// The baseline JPEG of a device BGR8 picture (include/vp_hip.h "the picture as a baseline JPEG"; kernels: kernels_misc.hip jpeg_*).  The host half --
// tables, header, bound -- needs no device.  JpegEncoder owns the device buffers of one user (a canvas, or one call of the operator entry) and grows
// them once per geometry: coefficients, interval lengths / offsets, the scan data at its bound, the Huffman entries, one pinned word for the total.
constexpr int kJpegDefaultRestart = 4;       // what restart_mcus = 0 selects (profiles/canvas_jpeg.txt)
constexpr size_t kJpegHeaderBytes = 629;     // SOI 2, APP0 18, DQT 2 x 69, SOF0 19, DHT 33 + 183 + 33 + 183, DRI 6, SOS 14: every segment has a fixed length
inline int jpeg_restart(int restart_mcus) { return restart_mcus == 0 ? kJpegDefaultRestart : restart_mcus; }
void jpeg_quant_tables(int quality, uint8_t q[2][64]);                 // luminance, chrominance; row-major
size_t jpeg_scan_bound(int h, int w, int restart_mcus);                // scan data alone, markers included
inline size_t jpeg_bound(int h, int w, int restart_mcus) { return kJpegHeaderBytes + jpeg_scan_bound(h, w, restart_mcus) + 2; }
void jpeg_write_header(int h, int w, int quality, int restart_mcus, uint8_t dst[kJpegHeaderBytes]);
class JpegEncoder {
 public:
  JpegEncoder() = default;
  ~JpegEncoder() { release(); }
  JpegEncoder(const JpegEncoder&) = delete;
  JpegEncoder& operator=(const JpegEncoder&) = delete;
  // d_bgr: h x w (both even, 2 .. 16384), rows pitch >= frame_bgr_pitch(w) apart, complete in `st`'s order.  Queues the four launches on st, waits for
  // the total, refuses a cap below the stream's size (std::invalid_argument naming it; *n = that size; dst beyond the header untouched), else copies the
  // scan data behind the header and waits again.  The device must be current.
  void encode(const uint8_t* d_bgr, int pitch, int h, int w, int quality, int restart_mcus, uint8_t* dst, size_t cap, size_t* n, const char* who, hipStream_t st);
  void release();

 private:
  void grow(void** p, size_t* cap, size_t bytes, hipStream_t st);
  int16_t* d_coef_ = nullptr;
  uint32_t* d_len_ = nullptr;
  uint8_t* d_out_ = nullptr;
  uint32_t* d_huff_ = nullptr;
  uint32_t* h_total_ = nullptr;
  size_t coef_cap_ = 0, len_cap_ = 0, out_cap_ = 0;
};

// vp_canvas (include/vp_hip.h; handle: vp_handle.hpp; kernels: kernels_misc.hip canvas_*): one BGR8 picture per camera frame on the device.  begin()
// copies a vp_frame's image; every engine, heads included, blends its mask or pastes its depth map into the region its input came from; the detector's
// boxes are drawn on top; fetch() hands the picture out once, in any vp_frame format.  The blend and the depth pipeline are those of
// Engine::visualize_mask / visualize_depth (same tables, same LUTs, same kernels or their region forms).  Owns its stream and buffers.
// The production display on top of that: overlay_lanes() (drawRawMasksInPlace's additive overlays from an EgoLanes engine's logits), draw_lane_rows()
// (an AutoSteer engine's valid rows, decided on the device) and fetch_resized() (the preprocess path's integer bilinear into a second picture).
// Ordering, all on the device: a draw makes the canvas's stream wait for the work queued on the engine's stream so far (the pass that wrote the mask),
// and makes the engine's stream wait for the canvas's read before anything queued on it later (the next pass) runs.  The only host waits are fetch(),
// sync(), a buffer that has to grow and the first use of a resize table of a new (source, destination) size: once per geometry.
class Canvas {
 public:
  explicit Canvas(int gpu);
  ~Canvas();
  Canvas(const Canvas&) = delete;
  Canvas& operator=(const Canvas&) = delete;
  void begin(const FrameView& f);   // the caller records the frame's consumer event behind it, on stream()
  void blend_mask(Engine& e, int viz_type);
  void blend_mask_u8(const uint8_t* mask, bool on_device, int mh, int mw, int viz_type, int x0, int y0, int w, int h);
  void paste_depth(Engine& e);
  void draw_boxes(const CanvasBox* boxes, int n);   // inclusive rectangles before clipping, in drawing order
  // the production display's lanes: one clamped additive overlay of up to kCanvasMaxPlanes fp32 planes (add_bgr: [n_planes][3]), and its engine form on the
  // three logit planes of a VP_EGOLANES engine
  void add_planes(const float* planes, bool on_device, int n_planes, int mh, int mw, float threshold, const uint8_t* add_bgr, int x0, int y0, int w, int h);
  void overlay_lanes(Engine& e, float threshold);
  void draw_points(const int* xy, int n, int radius, unsigned bgr);   // filled discs, clipped to the canvas
  void draw_lane_rows(Engine& e);                                     // a VP_AUTOSTEER engine's valid rows, read on the device
  void sync();
  // planes / strides / row_bytes / rows: what vp_canvas_layout answers for (format, h(), w()), checked by the caller
  void fetch(int format, uint8_t* const* planes, const int* strides, const size_t* row_bytes, const int* rows, int n_planes);
  // the same for the picture resized to out_h x out_w (the integer bilinear of the preprocess path); the canvas's own picture is left as it is
  void fetch_resized(int format, int out_h, int out_w, uint8_t* const* planes, const int* strides, const size_t* row_bytes, const int* rows, int n_planes);
  // the picture (out_h = 0), or the resized picture of fetch_resized, as a baseline JPEG; arguments checked by the caller.  Two host waits (JpegEncoder).
  void fetch_jpeg(int out_h, int out_w, int quality, int restart_mcus, uint8_t* dst, size_t cap, size_t* n);
  // vp_canvas_set_color (values checked by the caller): the standard and chroma rule of later fetches into the YUV formats and GRAY8
  void set_color(int matrix, int range, int chroma_mode) { matrix_ = matrix, range_ = range, chroma_mode_ = chroma_mode; }
  void get_color(int* matrix, int* range, int* chroma_mode) const { *matrix = matrix_, *range = range_, *chroma_mode = chroma_mode_; }
  hipStream_t stream() const { return stream_; }
  int gpu() const { return gpu_; }
  bool begun() const { return begun_; }
  int h() const { return h_; }
  int w() const { return w_; }
  int pitch() const { return pitch_; }
  uint8_t* device() const { return d_bgr_; }

 private:
  enum TableKind { kNearest = 0, kLinearF32 = 1, kLinearU8 = 2 };
  struct Table {
    int kind, src, dst;
    int* idx;      // nearest: [dst]; linear f32: [dst][2]; linear u8 (linear_taps_u8): [dst][4]
    float* wgt;    // linear f32: [dst][2]; else null
  };
  Table table(TableKind kind, int src, int dst);
  void release();
  enum Draws { kMaskOrDepth, kLanePlanes, kLaneRows };   // what a draw call needs of the engine: the kinds it accepts
  const Engine& source_of(Engine& e, const char* who, SourceRegion* r, Draws draws = kMaskOrDepth) const;
  void need_begun(const char* who) const;
  void wait_for(Engine& e);        // the canvas's stream behind the engine's work so far
  void release_to(Engine& e);      // the engine's later work behind the canvas's read
  void blend(const uint8_t* d_mask, int mh, int mw, int viz_type, const SourceRegion& r);
  void add(const float* d_planes, int n_planes, int mh, int mw, float threshold, const unsigned* add, const SourceRegion& r);
  void check_region(const char* who, int x0, int y0, int w, int h) const;
  const uint8_t* stage_host(const void* src, size_t bytes);   // a caller's pageable array: copied before the call returns, then one H2D into d_umask_
  void fetch_picture(const uint8_t* d_bgr, int pitch, int h, int w, int format, uint8_t* const* planes, const int* strides, const size_t* row_bytes, const int* rows,
                     int n_planes);
  int resize_to_small(int out_h, int out_w);   // queues the resize into d_small_; the row pitch of the result
  template <class T>
  void grow(T*& p, size_t& cap, size_t bytes);
  int gpu_;
  hipStream_t stream_ = nullptr;
  hipEvent_t ev_src_ = nullptr, ev_read_ = nullptr;
  uint8_t* d_bgr_ = nullptr;
  size_t bgr_cap_ = 0;
  int h_ = 0, w_ = 0, pitch_ = 0;
  bool begun_ = false;
  int matrix_ = 0, range_ = 0, chroma_mode_ = 0;   // BT.601, limited range, chroma of the even pixel
  std::vector<Table> tables_;
  uint8_t* d_lut_ = nullptr;       // [3 viz types][256][3], then viridis [256][3]
  unsigned* d_minmax_ = nullptr;   // [0, 2): the keys of the plane in work; [2, 4): their start values
  float* d_depth_ = nullptr;       // the depth plane at region size
  size_t depth_cap_ = 0;
  uint8_t* d_out_ = nullptr;       // fetch: the planes of the requested format
  size_t out_cap_ = 0;
  uint8_t* d_small_ = nullptr;     // fetch_resized: the resized picture, rows frame_bgr_pitch(out_w) apart
  size_t small_cap_ = 0;
  uint8_t* d_umask_ = nullptr;     // blend_mask_u8 / add_planes from the host: the caller's mask or planes
  size_t umask_cap_ = 0;
  uint8_t* h_umask_ = nullptr;     // ... staged through two pinned slots, as a frame upload is
  size_t h_umask_cap_ = 0;
  int umask_slot_ = 0;
  hipEvent_t umask_ev_[2] = {nullptr, nullptr};
  JpegEncoder jpeg_;               // fetch_jpeg: buffers of its own, never touched by the other fetches
};

// vp_metric (include/vp_hip.h; handle: vp_handle.hpp; kernels: kernels_misc.hip metric_*): the validation scores of the segmentation and depth trainers,
// one MetricRecord per frame in a device array of max_frames records.  An add_* call reads an engine's device-resident logits behind its pass (the
// canvas's ordering: wait_for / release_to), or a caller's tensors, queues the kernels on the metric's own stream and returns; fetch() is the one
// synchronisation.  Host waits besides it: a scratch or staging buffer that has to grow (once per geometry) and a pinned slot still being read by the
// copy queued two calls earlier.  Owns its stream and buffers.  One thread drives it.
class Metric {
 public:
  Metric(int gpu, int max_frames);
  ~Metric();
  Metric(const Metric&) = delete;
  Metric& operator=(const Metric&) = delete;
  void reset();
  // gt: u8 [h][w] of the engine's output size; gt_form 0 (class index) or 1 (bit c = plane c)
  void add_seg(Engine& e, const uint8_t* gt, bool gt_on_device, int gt_form);
  void add_depth(Engine& e, const float* gt, bool gt_on_device);
  void add_seg_pair(Engine& e, Engine& ref);
  void add_depth_pair(Engine& e, Engine& ref);
  void add_seg_logits(const float* logits, bool on_device, int c, int h, int w, const uint8_t* gt, bool gt_on_device, int gt_form);
  void add_depth_plane(const float* pred, bool pred_on_device, const float* gt, bool gt_on_device, int h, int w);
  int frames() const { return frames_; }
  int max_frames() const { return max_frames_; }
  void fetch(MetricRecord* out, int count);   // records [0, count), synchronous
  int gpu() const { return gpu_; }
  // the detector part (kernels.hpp DetValParams): records of its own, storage allocated by the first add_det*.  labels: host floats [n_labels][5]
  // (cls, cx, cy, w, h normalised to the network input), copied before the call returns
  void add_det(Engine& e, const float* labels, int n_labels, float conf, float iou, const float* iou_v, int n_iou);
  void add_det_pair(Engine& e, Engine& ref, float label_conf, float conf, float iou, const float* iou_v, int n_iou);
  void add_det_raw(const float* raw, bool on_device, int nc, int nb, int net_h, int net_w, const float* labels, int n_labels, float conf, float iou, const float* iou_v, int n_iou);
  int det_frames() const { return det_frames_; }
  int det_capacity() const { return max_frames_ < kDetFramesCap ? max_frames_ : kDetFramesCap; }
  // synchronous: the frame records, then rows and label classes up to the totals the device reports
  void fetch_det(std::vector<DetFrameRecord>* frames, std::vector<DetRowRecord>* rows, std::vector<float>* label_cls);
  int det_n_iou() const { return det_n_iou_; }
  static constexpr int kDetFramesCap = 16384, kDetLabelsPerFrame = 64;
  // the lane part (kernels.hpp MetricLanesParams / MetricRowsParams): records of their own, max_frames of each, storage allocated by the first add.
  // gt_form: kLanesGtPlanes (fp32 [3][h][w]), kLanesGtBits (u8 [h][w]) or kLanesGtBits4x (u8 [4h][4w])
  void add_lanes(Engine& e, const void* gt, bool gt_on_device, int gt_form);
  void add_lanes_pair(Engine& e, Engine& ref);
  void add_lanes_logits(const float* logits, bool on_device, int h, int w, const void* gt, bool gt_on_device, int gt_form);
  int lanes_frames() const { return lanes_frames_; }
  void fetch_lanes(LanesRecord* out, int count);
  // targets: host floats [64] each, copied before the call returns; thr: the run's table (another one is refused until reset())
  void add_rows(Engine& e, const float* target_xp, const float* target_h, const double* thr, int n_thr);
  void add_rows_pair(Engine& e, Engine& ref, const double* thr, int n_thr);
  void add_rows_raw(const float* xp, const float* hv, const float* target_xp, const float* target_h, int n_lines, int rows, const double* thr, int n_thr);
  int rows_lines() const { return rows_lines_; }
  int rows_n_thr() const { return rows_n_thr_; }
  const double* rows_thr() const { return rows_thr_; }
  void fetch_rows(RowsRecord* out, int count);
  // the label part (kernels.hpp LabelSegParams / LabelDepthParams): the ground truth is built on the device from a label file's decoded pixels, in host
  // memory and copied before the call returns; then the seg / depth chain of add_seg / add_depth.  One MetricRecord AND one LabelRecord per call, the
  // label records in storage of their own (allocated by the first such call).  crop: {l, t, r, b} or null (the whole image); colours: [n][4] r, g, b, class
  void add_seg_label(Engine& e, const uint8_t* label, int channels, int h, int w, int stride, const int* crop, const uint8_t* colours, int n_colours);
  void add_depth_label(Engine& e, const void* label, int dtype, int h, int w, int stride);
  void add_seg_logits_label(const float* logits, bool on_device, int c, int oh, int ow, const uint8_t* label, int channels, int h, int w, int stride, const int* crop,
                            const uint8_t* colours, int n_colours);
  void add_depth_plane_label(const float* pred, bool pred_on_device, int oh, int ow, const void* label, int dtype, int h, int w, int stride);
  int label_frames() const { return label_frames_; }
  void fetch_labels(LabelRecord* out, int count);

 private:
  struct Stage {   // a caller's pageable array: copied into one of two pinned slots before the call returns, then one H2D into `d`
    uint8_t* h = nullptr;
    size_t hcap = 0;
    uint8_t* d = nullptr;
    size_t dcap = 0;
    int slot = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
  };
  void release();
  template <class T>
  void grow(T*& p, size_t& cap, size_t bytes);
  const void* stage_host(Stage& s, const void* src, size_t bytes);
  const Engine& source_of(Engine& e, const char* who, bool depth) const;
  void wait_for(Engine& e, hipEvent_t ev);
  void release_to(Engine& e, hipEvent_t ev);
  MetricRecord* next_record(const char* who);
  void seg(const float* d_logits, const float* d_ref, const uint8_t* d_gt, int c, int h, int w, int gt_form, MetricRecord* rec);
  void depth(const float* d_pred, const float* d_gt, int h, int w, MetricRecord* rec);
  const Engine& det_source_of(Engine& e, const char* who) const;
  void det_begin(const char* who, int nc, int nb, int n_labels_bound, const float* iou_v, int n_iou, float conf, float iou);
  DetValParams det_chain(const float* d_raw, int nc, int nb, float conf, float iou, int which);
  void det_match(const float* d_labels, const unsigned* d_n_labels, int n_labels, int label_form, int net_h, int net_w);
  int gpu_, max_frames_, frames_ = 0;
  hipStream_t stream_ = nullptr;
  hipEvent_t ev_src_[2] = {nullptr, nullptr}, ev_read_[2] = {nullptr, nullptr};
  MetricRecord* d_records_ = nullptr;
  Stage stage_[2];   // [0] the prediction, [1] the ground truth
  uint8_t* d_scratch_ = nullptr;   // the depth chain's: see depth()
  size_t scratch_cap_ = 0;
  // detector part
  int det_frames_ = 0, det_n_iou_ = 0;
  size_t det_labels_bound_ = 0;      // labels added so far, at most (the pair form's count lives on the device)
  float det_iou_v_[kDetValMaxIou] = {};
  DetFrameRecord* d_det_frames_ = nullptr;
  DetRowRecord* d_det_rows_ = nullptr;
  float* d_det_label_cls_ = nullptr;
  uint8_t* d_det_small_ = nullptr;   // totals [2] | two sets of {rows [300][7], counts [3]} | pair labels [300][5] | their count
  uint8_t* d_det_scratch_ = nullptr; // the chain's keys, ranks, order, boxes
  size_t det_scratch_cap_ = 0;
  Stage det_stage_;                  // host labels
  // lane part
  const Engine& lanes_source_of(Engine& e, const char* who) const;
  const Engine& rows_source_of(Engine& e, const char* who) const;
  LanesRecord* lanes_next(const char* who);
  void lanes(const float* d_logits, const void* d_gt, int gt_form, int h, int w, LanesRecord* rec);
  RowsRecord* rows_next(const char* who, int n_lines, const double* thr, int n_thr);
  void rows(const float* xp, const float* hv, const float* txp, const float* thv, int n_lines, int n_rows, RowsRecord* rec);
  int lanes_frames_ = 0, rows_lines_ = 0, rows_n_thr_ = 0;
  double rows_thr_[kMetricRowsMaxThr] = {};
  LanesRecord* d_lanes_records_ = nullptr;
  RowsRecord* d_rows_records_ = nullptr;
  uint8_t* d_lanes_scratch_ = nullptr;   // the partials, then the general path's D0 and pooled levels: see lanes()
  size_t lanes_scratch_cap_ = 0;
  // label part
  struct LabelTab {   // a nearest table on the device, kept per (source, destination) size as Canvas::table keeps its tables
    int src, dst;
    int* idx;
  };
  const int* label_tab(int src, int dst);
  LabelRecord* label_next(const char* who);
  const uint8_t* label_seg(LabelSegParams q, const uint8_t* label, int oh, int ow, LabelRecord* rec);
  const float* label_depth(const void* label, int dtype, int h, int w, int stride, int oh, int ow, LabelRecord* rec);
  int label_frames_ = 0;
  LabelRecord* d_label_records_ = nullptr;
  uint8_t* d_label_scratch_ = nullptr;   // the ground truth at output size, then the partials
  size_t label_scratch_cap_ = 0;
  std::vector<LabelTab> label_tabs_;
};

// vp_lanes (include/vp_hip.h; handle: vp_handle.hpp; kernel: kernels_detect.hip lane_filter_kernel): the production app's LaneFilter::update behind an
// EgoLanes pass.  add() queues one lane_filter launch on the filter's own stream, ordered against the engine by events alone (Metric's wait_for /
// release_to), into the next of `capacity` device records (a ring); fetch() is the one synchronisation: it copies the oldest pending records and, in
// the order they were added, solves each lane's normal equations from the integer moments (lanes_fit) and applies the temporal smoothing, whose state
// (the previous fit of either lane) lives here on the host.  The collected points stay in a device side buffer until fetch_points asks for them.
// Owns its stream and buffers.  One thread drives it.
struct LanesFit {
  int order;            // 0: no fit (no start point, fewer than 4 points, or singular), 1: a line, 2: a quadratic
  int flags;            // kLanesSingular | kLanesSmoothed
  int coeffs_valid;     // coeffs holds what LaneFilter::update leaves in left_coeffs / right_coeffs
  double raw[6];        // this frame's own fit: 0, a, b, c, min_y, max_y of x = a y^2 + b y + c
  double coeffs[6];     // the fit blended with the previous frame's
};
constexpr int kLanesSingular = 1, kLanesSmoothed = 2;
// the least-squares polynomial of `order` (1 or 2) from the moments S_k = sum y^k, T_k = sum x y^k: out = {a, b, c} (a = 0 for a line).  Cramer's rule
// with the determinants exact in 128-bit integers and each coefficient ONE correctly rounded quotient.  Returns false (out untouched) when the system is
// singular.  Every |S_k|, |T_k| must be below 2^40 (std::invalid_argument): the production moments stay below 2^37.
bool lanes_fit(const long long S[5], const long long T[3], int order, double out[3]);

class Lanes {
 public:
  Lanes(int gpu, int capacity);
  ~Lanes();
  Lanes(const Lanes&) = delete;
  Lanes& operator=(const Lanes&) = delete;
  void set_smoothing(float s) { smoothing_ = s; }
  void reset();                                        // forgets both previous fits; refused while records are pending
  void add(Engine& e, float threshold);                // a VP_EGOLANES engine (a shared-prefix head included) with a pass behind it
  void add_logits(const float* host, float threshold); // fp32 [3][80][160] in host memory, copied before the call returns
  int pending() const { return count_; }
  int capacity() const { return capacity_; }
  int gpu() const { return gpu_; }
  // the oldest `count` (<= pending) records, then their fits [count][2] in order; they stop being pending
  void fetch(LaneFilterRecord* recs, LanesFit* fits, int count);
  // the point list of one lane of pending record `index` (oldest first), the upward run's then the downward run's: xy [n][2] bytes; returns n
  int fetch_points(int index, int lane, uint8_t* xy, int max_points);

 private:
  void release();
  LaneFilterRecord* next_record(const char* who);
  void launch(const float* d_logits, float threshold);
  int gpu_, capacity_, head_ = 0, count_ = 0;
  float smoothing_ = 0.5f;
  hipStream_t stream_ = nullptr;
  hipEvent_t ev_src_ = nullptr, ev_read_ = nullptr, stage_ev_[2] = {nullptr, nullptr};
  LaneFilterRecord* d_records_ = nullptr;
  LaneFilterRecord* h_records_ = nullptr;   // pinned [capacity]: where fetch lands the records
  uint16_t* d_points_ = nullptr;     // [capacity][2 lanes][2 runs][kLaneRunPoints]
  float* d_stage_ = nullptr;         // add_logits: the caller's planes on the device ...
  float* h_stage_ = nullptr;         // ... staged through two pinned slots
  int stage_slot_ = 0;
  struct Prev {
    bool valid = false;
    double c[6] = {};
  } prev_[2];
};

// the arguments of a colour / mask label checked and laid into the kernel's parameters (std::invalid_argument names `who`); label, tables, outputs unset
LabelSegParams label_seg_params(const char* who, const void* label, int channels, int h, int w, int stride, const int* crop, const uint8_t* colours, int n_colours);
void label_check_depth(const char* who, const void* label, int dtype, int h, int w, int stride);
// OpenCV's resizeNN index table (oracle/pre_post.py nearest_index): tab[d] for d in [0, dst)
void label_nearest_tab(int src, int dst, int* tab);

#define VP_HIP_CHECK(expr)                                                                                   \
  do {                                                                                                       \
    hipError_t _e = (expr);                                                                                  \
    if (_e != hipSuccess)                                                                                    \
      throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(_e) + " at " #expr);           \
  } while (0)

}  // namespace vp

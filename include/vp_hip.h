/*
 * vp_hip.h -- C ABI of libvp_hip.so: MI355X-native (gfx950) engine for the VisionPilot per-frame hot path
 *             preprocess -> SceneSeg / Scene3D / DomainSeg / EgoLanes forward -> argmax / threshold decode.
 *
 * This is the drop-in boundary.  Plain pointers and sizes only; no exceptions cross it.
 * Reference interfaces each entry point replaces (paths relative to the reference repo):
 *
 *   vp_create / vp_create_from_memory
 *       OnnxRuntimeBackend::OnnxRuntimeBackend(model_path, precision, gpu_id)
 *         VisionPilot/middleware_recipes/common/backends/onnx_runtime_backend.cpp:9-39
 *       TensorRTBackend ctor            .../common/backends/tensorrt_backend.cpp:35-60
 *       EgoLanesOnnxEngine ctor         VisionPilot/production_release/src/inference/onnxruntime_engine.cpp:13-66
 *       SceneSegNetworkInfer.__init__   Models/inference/scene_seg_infer.py:12-36
 *   vp_infer
 *       InferenceBackend::doInference(const cv::Mat&)  .../common/include/inference_backend_base.hpp:19,
 *         onnx_runtime_backend.cpp:41-82 (preprocess + Run)
 *       EgoLanesOnnxEngine::doInference onnxruntime_engine.cpp:104-135 (+ preprocessEgoLanes :72-102)
 *   vp_infer_tensor
 *       XInfer.inference() after ToTensor/Normalize   Models/inference/scene_seg_infer.py:44-49
 *   vp_logits
 *       InferenceBackend::getRawTensorData / getTensorShape   inference_backend_base.hpp:22-23
 *   vp_input_hw
 *       getModelInputHeight / getModelInputWidth              inference_backend_base.hpp:25-26
 *   vp_mask_u8 (VP_DECODE_*)
 *       RunModelNode::onImage argmax / threshold loops  ROS2/models/src/run_model_node.cpp:144-171
 *       MasksVisualizationKernels::createMaskFromTensor{CUDA,HIP}, createEgoLanesMaskFromTensorCUDA
 *         common/visualizers/cuda_visualization_kernels.cu:13-75, masks_viz.hip.cpp:11-97
 *       torch.max(dim=2)                                 Models/inference/scene_seg_infer.py:52-55
 *   vp_mask_resized_u8 / vp_depth_resized_f32
 *       cv::resize(mask, INTER_NEAREST) / cv::resize(depth, INTER_LINEAR)  run_model_node.cpp:104,177
 *
 * Threading: one engine per caller thread; an engine owns its HIP stream, every buffer it uses and its kernel plan, so several
 * engines may live in one process and be created / driven from different threads concurrently.  Process-wide
 * state, all of it optional and each behind its own mutex: (1) the developer options of vp_set_option (read when an engine's plan
 * is built; no production path sets one); (2) the frame pools of vp_register_frames (a table of page-locked ranges, consulted per
 * upload); (3) RCCL's dlopen handle (vp_comm_*).  Nothing an engine computes depends on another engine's existence.
 * All functions return 0 on success and a negative vp_status on failure; vp_last_error() gives the text.
 */
#ifndef VP_HIP_H_
#define VP_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vp_engine vp_engine;

enum vp_status { VP_OK = 0, VP_ERR_ARG = -1, VP_ERR_WEIGHTS = -2, VP_ERR_HIP = -3, VP_ERR_STATE = -4,
                 VP_ERR_RANGE = -5 /* a value left the fp16 range the matrix pipe carries: see vp_set_finite_check */ };

/* VP_AUTODRIVE (BASELINE configs[4]): Models/model_components/autodrive/autodrive_network.py:32-36 --
 * shared backbone on the previous and the current frame (network input 1x3x512x1024, RGB planes), head -> three scalars
 * returned through vp_logits as shape {1,3,1,1} = (d_norm, curvature, flag_logit); no mask. */
/* VP_AUTOSPEED: the detector network, Models/model_components/auto_speed/auto_speed_network.py:33-48, version 'n' (the number of
 * classes is read from the weights; 4 in the reference's checkpoints).  Input: 1x3x512x1024 fp32 planes R, G, B in [0, 1], no mean / std -- what
 * vp_detect_preprocess leaves on the device; the engine has NO frame preprocess of its own: its entries are vp_infer_tensor (host tensor) and
 * vp_detect_infer (below); vp_infer / vp_upload_frame return VP_ERR_STATE.  Output through vp_logits: shape {1, 4 + nc, 1, 10752} = the head's
 * eval-mode tensor [4 + nc][10752] (cx, cy, w, h in input pixels, then sigmoid class scores; levels of stride 8, 16, 32 one after the other), the
 * tensor vp_detect_postprocess reads; no mask.  VP_FP16 / VP_FP16X3 (| VP_PLAN_LATENCY; VP_FP16X3 also | VP_ACT_SCALE: vp_calibrate_range then runs on
 * the tensor of the last vp_infer_tensor / vp_detect_infer, and vp_detect_infer works unchanged on the calibrated engine); VP_WEIGHTS_FP8,
 * vp_create_shared* and vp_create_batched* are refused with VP_ERR_ARG. */
/* VP_AUTOSTEER: the AutoSteer 2.0 lane-perception network, Models/model_components/auto_steer/auto_steer_network.py:39-43, version 'n' (what
 * Models/inference/auto_steer_infer.py AutoSteerNetworkInfer runs).  Input: a 512 x 1024 frame taken as it is -- R, G, B planes of u8 / 255, no mean / std,
 * no resize (auto_steer_infer.py:19-23,41-45): vp_infer / vp_upload_frame return VP_ERR_ARG for any other geometry (the reference raises ValueError),
 * vp_set_input_format picks BGR8 (default) or RGB8 bytes, vp_infer_tensor takes the [3][512][1024] planes.  Output through vp_logits: shape
 * {1, 2, 64, 1}: plane 0 = xp (ego-lane position per feature row, in [0, 1)), plane 1 = h_vector (per-row validity; the visualisation draws a row when
 * it is >= 0.5); no mask.  VP_FP16 / VP_FP16X3 (| VP_PLAN_LATENCY; VP_FP16X3 also | VP_ACT_SCALE: vp_calibrate_range then runs on the resident
 * frame); VP_WEIGHTS_FP8, vp_create_shared* and vp_create_batched* are refused with VP_ERR_ARG; a blob whose head is not the 'n' head is refused with
 * VP_ERR_WEIGHTS naming the key.  (The v1 temporal AutoSteer head fed by EgoLanes logits is another model and not part of this library:
 * vp_set_lane_ring hands its input over.) */
enum vp_model_kind { VP_SCENESEG = 0, VP_SCENE3D = 1, VP_DOMAINSEG = 2, VP_EGOLANES = 3, VP_AUTODRIVE = 4, VP_AUTOSPEED = 5, VP_AUTOSTEER = 6 };

/* VP_FP16  : fp16 tensors, fp16 MFMA, fp32 accumulate (the reference's "fp16" configuration).
 * VP_FP16X3: fp32-class accuracy on the fp16 matrix pipe: every tensor is a (hi, lo) fp16 pair and every
 *            product is three MFMAs (hi*hi + hi*lo + lo*hi), fp32 accumulate -- the parity mode (1e-3). */
enum vp_precision { VP_FP16 = 0, VP_FP16X3 = 1,
                    /* OR-able flag: every conv / linear weight is quantised at load to per-output-row OCP e4m3 (fp8) (BASELINE
                     * configs[4] "fp8 weights"; the reference's PTQ flow: Models/exports/quantization/PTQ/AutoDrive).  Round 4: it is
                     * STORAGE, not only numerics -- on the kernels that stage weights through registers (the generic GEMM kernel, the
                     * 3x3 halo kernel, the FC kernel: every matrix / FC layer of VP_AUTODRIVE) HBM holds one e4m3 byte per weight plus
                     * a per-row fp32 scale; the staging path converts 8 codes -> 8 fp16 values on their way to LDS (exact: every e4m3
                     * value is an fp16 value) and the epilogue applies the scale to the fp32 accumulator.  The arithmetic stays the
                     * fp16 matrix pipe with fp16 / (hi, lo) activations (fp8 MFMA would quantise the ACTIVATIONS to 3 mantissa bits:
                     * outside the 1e-3 bar).  Layers on the LDS-DMA / register-stationary kernels of the scene networks keep
                     * de-quantised fp16 planes.  vp_weight_bytes reports the split. */
                    VP_WEIGHTS_FP8 = 16,
                    /* OR-able flag (round 6): the LATENCY kernel plan for THIS engine.  The default plan spends a layer's own latency where the rest
                     * of the frame can use the CUs it frees (forked heads on one camera, several cameras per GPU); a host that runs ONE network on
                     * ONE camera, one frame at a time, has nothing to put there and gets 3-7 % of its frame back with this flag.  Per engine: a
                     * process that holds several engines (VisionPilot/production_release/main.cpp:505-535: EgoLanes beside AutoSpeed / AutoSteer)
                     * chooses for each; results differ from the default plan's only in fp32 summation order; vp_plan_hash() tells the plans apart.
                     * A shared-prefix engine may choose differently from its base. */
                    VP_PLAN_LATENCY = 32,
                    /* OR-able flag: per-tensor power-of-two ACTIVATION SCALE (see RANGE GUARD below).  VP_AUTODRIVE, VP_AUTOSPEED and VP_AUTOSTEER
                     * (the YOLO-block family) with VP_FP16X3 only, alone or with VP_PLAN_LATENCY (VP_AUTODRIVE also with VP_WEIGHTS_FP8); the scene
                     * network kinds, VP_FP16, vp_create_shared* and vp_create_batched* return VP_ERR_ARG.  Every activation tensor t is stored as
                     * x * 2^-s_t; all s_t start at 0, and with all of them 0 the engine's launches and bits are the unflagged engine's.
                     * vp_calibrate_range chooses them, vp_set_act_scales installs a shipped table. */
                    VP_ACT_SCALE = 64,
                    /* OR-able flag: the e4m3 MFMA form of the big plain 3x3 layers (see FP8 MFMA ENGINES below).  With VP_FP16 only, alone or with
                     * VP_PLAN_LATENCY, for VP_SCENESEG, VP_SCENE3D, VP_DOMAINSEG and VP_EGOLANES engines that own their whole network; VP_FP16X3,
                     * VP_WEIGHTS_FP8, VP_ACT_SCALE, the other three kinds, vp_create_shared* and vp_create_batched* return VP_ERR_ARG and say which.
                     * An engine without the flag is untouched: same plan, same bits. */
                    VP_MFMA_FP8 = 128 };

enum vp_pixel_format { VP_BGR8 = 0, VP_RGB8 = 1 };
/* Plane order of the network input: BGR planes = middleware "common" backends (onnx_runtime_backend.cpp:47-57),
 * RGB planes = EgoLanes engines and the Python wrappers.  Normalisation constants follow the plane's colour. */
enum vp_plane_order { VP_PLANES_BGR = 0, VP_PLANES_RGB = 1 };

enum vp_decode_mode {
  VP_DECODE_SEG_MASK = 0,   /* C>1: 255 where argmax==1 else 0 ; C==1: 255 where logit>0 */
  VP_DECODE_LANE_LABEL = 1, /* {2,1,0,255} priority label */
  VP_DECODE_CLASS_INDEX = 2 /* raw argmax index (first maximum wins) */
};

/* ---- lifetime ------------------------------------------------------------------------------------------
 * weights_path: a VPW1 blob (autoware_vision_pilot_amd/weights.py) or -- as the reference's backends take
 * (`model_path: *.onnx`, ROS2/models/config/autoseg.yaml:3; OnnxRuntimeBackend ctor onnx_runtime_backend.cpp:14-38) --
 * an `.onnx` file made by Models/exports/convert_pytorch_to_onnx.py:144-154.  ONNX files are read by the library's own
 * wire-format parser (csrc/onnx_reader.cpp): weights only, the graph is the engine's. */
int vp_create(vp_engine** out, int model_kind, const char* weights_path, int precision, int gpu_id, char* err, size_t err_len);
int vp_create_from_memory(vp_engine** out, int model_kind, const void* blob, size_t blob_bytes, int precision, int gpu_id,
                          char* err, size_t err_len);
void vp_destroy(vp_engine* e);
const char* vp_last_error(const vp_engine* e);
/* Host only (no HIP device needed): ONNX file -> VPW1 blob file, the conversion vp_create does in memory. */
int vp_convert_onnx(const char* onnx_path, const char* vpw_path, char* err, size_t err_len);

/* ---- shared-prefix engines (BASELINE configs[2]: SceneSeg + Scene3D + EgoLanes on one camera) -----------
 * The reference builds Scene3D and DomainSeg ON a pre-trained SceneSeg: Scene3DNetwork wraps its backbone
 * (Models/model_components/scene_3d_network.py:9-13, pre_trained_backbone.py), DomainSegNetwork its backbone +
 * context + neck (domain_seg_network.py:9-12, domain_seg_upstream.py), but every ONNX/TensorRT backend instance
 * re-runs that prefix per model.  vp_create_shared builds an engine whose plan STARTS from the base engine's feature
 * tensors: sub-networks whose parameters are byte-identical to the base's are not rebuilt or re-run
 * (vp_shared_level: 1 = backbone, 2 = backbone + context + neck).  It runs on the base engine's stream:
 *     vp_infer(base, frame, ...);  vp_infer_shared(head2);  vp_infer_shared(head3);
 * Errors: VP_ERR_ARG if the backbone parameters differ, if precision / gpu differ from the base, or if the base is
 * itself a shared engine.  The base must outlive its shared engines; a shared engine accepts no frames of its own. */
int vp_create_shared(vp_engine** out, vp_engine* base, int model_kind, const char* weights_path, int precision, int gpu_id,
                     char* err, size_t err_len);
int vp_create_shared_from_memory(vp_engine** out, vp_engine* base, int model_kind, const void* blob, size_t blob_bytes,
                                 int precision, int gpu_id, char* err, size_t err_len);
int vp_shared_level(const vp_engine* e);
int vp_infer_shared(vp_engine* e);

/* ---- batched encoder (multi-camera rigs, BASELINE configs[2]/[3]: several cameras per GPU) -----------------
 * Every backend instance of the reference runs batch 1 (onnx_runtime_backend.cpp:59, tensorrt_backend.cpp:124), one
 * instance per camera.  The EfficientNet encoder is ~100 latency-sized launches per frame; a batched encoder engine runs
 * preprocess + encoder for `frames` cameras per pass (activations [frames][H][W][C]: 1x1 convolutions as one GEMM over all
 * pixels, depthwise + squeeze-excite kernels with the frame on a grid axis, the SE-gated projections per frame) and owns no
 * context / neck / head.  Each camera's head is a shared-prefix engine on its slot:
 *     vp_create_batched(&enc, VP_SCENESEG, "SceneSeg.onnx", VP_FP16, gpu, 3, ...);
 *     for f in 0..2: vp_create_shared_frame(&head[f], enc, f, VP_SCENESEG, "SceneSeg.onnx", VP_FP16, gpu, ...);
 *     per pass: vp_upload_frame_n(enc, f, frame_f, h, w, stride) x3;  vp_enqueue(enc);  vp_infer_shared(head[f]) x3.
 * All frames of a pass share one geometry.  Errors as for vp_create_shared; frames in 1..16.  Per camera the results equal
 * the single-frame engine's up to fp32 summation order (the split-K factor of a 1x1 GEMM follows its pixel count, which the
 * batch multiplies; measured bit-identical on the tested networks, the tests hold them to 1e-3).  Timed in DESIGN.md.
 * vp_upload_frame* stages pageable frames through two pinned slots: a slot is rewritten only after the H2D copy that last read it
 * has completed (per-slot event), so any number of uploads may be queued without a synchronisation in between. */
int vp_create_batched(vp_engine** out, int model_kind, const char* weights_path, int precision, int gpu_id, int frames, char* err,
                      size_t err_len);
int vp_create_batched_from_memory(vp_engine** out, int model_kind, const void* blob, size_t blob_bytes, int precision, int gpu_id,
                                  int frames, char* err, size_t err_len);
int vp_create_shared_frame(vp_engine** out, vp_engine* base, int frame_index, int model_kind, const char* weights_path, int precision,
                           int gpu_id, char* err, size_t err_len);
int vp_create_shared_frame_from_memory(vp_engine** out, vp_engine* base, int frame_index, int model_kind, const void* blob,
                                       size_t blob_bytes, int precision, int gpu_id, char* err, size_t err_len);
int vp_frames(const vp_engine* e);
int vp_upload_frame_n(vp_engine* e, int index, const uint8_t* frame, int h, int w, int stride_bytes);

/* ---- configuration ------------------------------------------------------------------------------------- */
int vp_set_input_format(vp_engine* e, int pixel_format, int plane_order);
int vp_set_decode_mode(vp_engine* e, int decode_mode);
/* How a frame of another size reaches the network's input size.  VP_RESIZE_CV_LINEAR (default of the scene networks): the integer
 * bilinear modelled on cv::resize INTER_LINEAR, what the C++ nodes do (onnx_runtime_backend.cpp:44).  VP_RESIZE_PIL_BILINEAR
 * (default of VP_AUTODRIVE) / VP_RESIZE_PIL_BICUBIC: Pillow's antialiased Image.resize, bit-exact against Pillow 12.2 -- the
 * Python scripts' frame path (Models/visualizations/AutoDrive/video_visualization.py:29-33 BILINEAR; the scene networks'
 * visualisation scripts call Image.resize((640, 320)) with Pillow's default filter, BICUBIC).  VP_ERR_ARG on a shared engine. */
enum vp_resize_mode { VP_RESIZE_CV_LINEAR = 0, VP_RESIZE_PIL_BILINEAR = 1, VP_RESIZE_PIL_BICUBIC = 2 };
int vp_set_resize_mode(vp_engine* e, int resize_mode);
int vp_get_resize_mode(const vp_engine* e);
/* host only: one axis' tap tables of the VP_RESIZE_PIL_* modes -- bounds[out][2] = {first source index, taps}, coeffs[out][ksize] with
 * 22 fractional bits; returns ksize (> 0) or VP_ERR_ARG (coeffs_cap < out_size * ksize ints).  For tests / external checks. */
int vp_resample_coeffs(int in_size, int out_size, int resize_mode, int* bounds, int* coeffs, int coeffs_cap);
/* The u8 -> [0, 1] step ahead of (x - mean) / std exists in two spellings that differ in the last bit for 322 of the 768 (byte, channel)
 * pairs (<= 7.2e-7): VP_NORM_TORCHVISION q / 255 -- torchvision's to_tensor, the Python operator API (Models/inference/scene_seg_infer.py:
 * 15-20; default) -- and VP_NORM_OPENCV q * fl(1/255) -- cv::Mat::convertTo(CV_32FC3, 1.0 / 255.0) of the C++ front-ends
 * (onnx_runtime_backend.cpp:45-49, tensorrt_backend.cpp:164-168, production_release onnxruntime_engine.cpp:85,94-100), which
 * adapters/hip_backend.hpp and adapters/egolanes_hip_engine.hpp select.  VP_ERR_ARG on a shared engine. */
enum vp_norm_form { VP_NORM_TORCHVISION = 0, VP_NORM_OPENCV = 1 };
int vp_set_norm_form(vp_engine* e, int norm_form);
int vp_get_norm_form(const vp_engine* e);
int vp_get_decode_mode(const vp_engine* e);      /* the vp_decode_mode in force (>= 0), or VP_ERR_ARG */
int vp_gpu_id(const vp_engine* e);               /* the device the engine lives on */
int vp_device_count(void);                       /* GPUs visible to this process (0 = none): a thread-per-GPU host sizes its world with it */
int vp_host_logits_current(const vp_engine* e);  /* 1 = the host pointer vp_logits() hands out holds the LAST pass's logits */
int vp_input_hw(const vp_engine* e, int* h, int* w);

/* Which outputs vp_infer / vp_infer_shared / vp_infer_multi copy to the host before they return (default both, what
 * TensorRTBackend::doInference does: tensorrt_backend.cpp:184-199).  A de-selected output stays in HBM and is copied on the
 * first vp_logits / vp_mask_u8 call instead: a host that only consumes the decoded mask (RunModelNode publishes the mask,
 * run_model_node.cpp:173-190) saves the 2.4 MB fp32 logits transfer per frame. */
enum vp_output_bits { VP_OUT_LOGITS = 1, VP_OUT_MASK = 2 };
int vp_set_outputs(vp_engine* e, int output_bits);
/* vp_infer stages the caller's pageable frame through a pinned double buffer owned by the engine (default 1). */
int vp_set_pinned_staging(vp_engine* e, int enable);
/* FRAME POOLS (round 5).  The staging above is a single-threaded host memcpy of the whole frame (2.76 MB at 1280x720: ~130 us of a 3.5 ms
 * node frame).  A host that owns its frame buffers (a cv::Mat pool, a camera ring, a ROS message arena) registers them ONCE:
 *   vp_register_frames(pool, bytes)  page-locks [pool, pool + bytes) for DMA (hipHostRegister, portable across devices); process-wide;
 * and every vp_infer* / vp_upload_frame* whose frame lies wholly inside a registered range is then copied by ONE DMA straight from the
 * caller's memory -- no staging copy.  Contract for the asynchronous calls (vp_upload_frame*): such a frame must stay unmodified until the
 * pass that consumes it has been synchronised (vp_sync / vp_fetch_outputs / vp_infer*); the staged path copied it before returning, this one
 * does not.  The synchronous vp_infer* calls return after the copy, as before.  Frames outside every registered range take the staged path.
 * What TensorRTBackend does with its own pinned input buffer (tensorrt_backend.cpp:184-186), offered to the caller's buffers instead.
 * vp_unregister_frames(pool) releases a range registered with exactly that pointer (after the last pass that read it was synchronised).
 * Returns VP_ERR_ARG (null / zero / overlapping an existing range / unknown pointer) or VP_ERR_HIP (the runtime refused to lock the pages).
 * Device context: the range is registered PORTABLE (usable from every device); the call itself runs on the calling thread's current HIP device
 * (device 0 for a thread that never called hipSetDevice) -- a host may call it before or after vp_create, from any thread. */
int vp_register_frames(const void* pool, size_t bytes);
int vp_unregister_frames(const void* pool);
/* {1, C, H, W} of the output tensor WITHOUT touching the device: vp_logits also returns the shape but fetches a de-selected tensor
 * (vp_set_outputs) on the way.  Same state rule as vp_logits: VP_ERR_STATE before the first inference (onnx_runtime_backend.cpp:86-91). */
int vp_output_shape(const vp_engine* e, int64_t shape[4]);
int vp_output_dims(const vp_engine* e, int64_t shape[4]);  /* the same shape, answered from creation on (vp_output_shape: VP_ERR_STATE before the first inference) */
/* ACTIVATION SCALE (engines created with VP_ACT_SCALE; closes the RANGE GUARD's per-frame case below for AutoDrive, AutoSpeed and AutoSteer).
 * vp_calibrate_range: runs the plan eagerly, launch by launch, over the RESIDENT frame -- AutoDrive: after vp_infer_pair (whatever it returned) over that
 *   pair, after vp_upload_frame over that frame as both halves of the pair; AutoSteer: over the frame of the last vp_upload_frame / vp_infer; AutoSpeed:
 *   over the input tensor of the last vp_infer_tensor / vp_detect_infer (single-frame plans: one pass, nothing parked) -- measures every tensor a launch
 *   stores and moves its exponent so that the stored abs-max lies in [2^(target_log2 - 1), 2^target_log2); target_log2 1 .. 15, 0 = 12 (16x headroom
 *   below 65504).  A tensor that holds inf / NaN gets +16, at most 3 times, else VP_ERR_RANGE names it.  Later calls only RAISE exponents (calibrate
 *   over several frames: the per-tensor maximum); vp_reset_range puts all back to 0.  AutoDrive only (the other two kinds keep nothing from one frame
 *   to the next): the stream continues behind a calibration -- the current frame's features stay parked, so the next vp_infer pairs with it; behind
 *   vp_set_act_scales and vp_reset_range the next vp_infer is the first frame of a stream; a vp_upload_frame or vp_infer after the pair drops the
 *   pair's previous frame.
 * vp_act_scales / vp_set_act_scales: the table, one exponent per vp_tensor_count() entry, so a host calibrates once and ships it: engines with equal
 *   tables give equal bits.  VP_ERR_ARG if n differs or if tensors that share storage (alias slices, copies, max-pools) disagree.  An installed exponent counts as measured: a later calibration only raises it.  vp_plan_hash does not change: exponents are data, not plan.
 * vp_tensor_read and vp_logits return true values.  The range probe stays on: a frame beyond the calibrated headroom still returns VP_ERR_RANGE. */
int vp_calibrate_range(vp_engine* e, int target_log2);
int vp_reset_range(vp_engine* e);
int vp_act_scales(const vp_engine* e, int* exps, int cap);   /* returns the tensor count */
int vp_set_act_scales(vp_engine* e, const int* exps, int n);
/* FP8 MFMA ENGINES (engines created with VP_FP16 | VP_MFMA_FP8).  The VP_FP16 engines are the non-parity configuration (judged by a 3e-2 regression
 * bound and by the task scores of vp_metric, not by 1e-3); the flag moves their big plain 3x3 layers -- 3x3, stride 1, conv + bias + {GELU, none}, one
 * input tensor, input channels a multiple of 64, output channels that pad to a multiple of 64 without waste, maps of H * W >= 12800 pixels (80 x 160 and
 * larger) and, as measured, at least 512 input channels: decode_layer_5 of the scene decoders; decode_layer_7 / 9 fit the kernel but run faster on their
 * fp16 kernels (profiles/f8_mfma.txt) and stay there -- onto v_mfma_scale_f32_32x32x64_f8f6f4 with e4m3 operands, the one fp8 MFMA that runs at twice
 * the fp16 rate.  vp_layer_kernel reports "conv3x3_f8" for those launches; every other launch is the unflagged plan's.
 * THE QUANTISATION RULE of such a layer (restated in numpy in tests/f8_cases.py):
 *   activations: the stored fp16 value x of the input tensor becomes q = e4m3(x * 2^-qexp), qexp a per-layer integer in [-24, 24] (the scaling is
 *     exact).  e4m3 is OCP e4m3fn (bias 7, maximum 448, subnormals down to 2^-9; not the fnuz encoding); rounding is to nearest, ties to even; every
 *     finite or infinite value that would round above 448 gives +-448; NaN gives the NaN code (0x7f with the sign); zeros keep their sign.
 *   weights: per output channel n the e4m3 codes of w / S_n and the fp32 row scale S_n = amax_n / 448 (1 for an all-zero row): what
 *     vp_fp8_encode_rows returns (the packer of VP_WEIGHTS_FP8).
 *   result: y_n = fl32(acc_n * fl32(S_n * 2^qexp)) + bias_n, acc_n the fp32 MFMA accumulator over the e4m3 products; then the layer's activation
 *     and the engine's fp16 store.
 * vp_calibrate_fp8: one eager pass over the RESIDENT frame (the walk of vp_range_survey); for every fp8 layer, in plan order and before the layer runs,
 *   qexp is set so that absmax(input) * 2^-qexp lies in [2^(target_log2 - 1), 2^target_log2) -- target_log2 1 .. 8, 0 = 8 (1.75x headroom below 448),
 *   clamped to [-24, 24].  An all-zero input keeps its qexp.  Later calls only RAISE (calibrate over several frames); vp_reset_fp8 puts every qexp back
 *   to 0.  All qexp start at 0.  VP_ERR_STATE when nothing is resident.
 * vp_fp8_layers: out[i], i < min(cap, count), for the i-th conv3x3_f8 launch in plan order; returns the count.
 * vp_set_fp8_exps: installs a shipped table, one exponent per entry of vp_fp8_layers (VP_ERR_ARG if n differs or an exponent is outside [-24, 24]);
 *   an installed exponent counts as measured.  Engines with equal tables give equal bits; vp_plan_hash does not change (exponents are data, not plan);
 *   a changed exponent re-captures the graph on the next pass.
 * All four return VP_ERR_ARG on an engine created without the flag. */
typedef struct vp_fp8_layer {
  int launch;   /* index of the launch (vp_layer_name / vp_layer_kernel) */
  int tensor;   /* index of its input tensor (vp_tensor_info, vp_tensor_read, vp_range_survey) */
  int qexp;
} vp_fp8_layer;
int vp_calibrate_fp8(vp_engine* e, int target_log2);
int vp_reset_fp8(vp_engine* e);
int vp_fp8_layers(const vp_engine* e, vp_fp8_layer* out, int cap);
int vp_set_fp8_exps(vp_engine* e, const int* exps, int n);
/* host only: codes[i] = the e4m3 code the rule above gives the fp16 bit pattern f16[i] under exponent qexp (|qexp| <= 24, else VP_ERR_ARG) */
int vp_fp8_quantize_act(const uint16_t* f16, size_t n, int qexp, uint8_t* codes);
/* RANGE SURVEY (any engine that owns its whole network: all seven kinds, VP_FP16 and VP_FP16X3, with or without VP_WEIGHTS_FP8 / VP_PLAN_LATENCY /
 * VP_ACT_SCALE).  vp_range_survey runs the plan eagerly, launch by launch, over the RESIDENT input -- the frame of the last vp_upload_frame / vp_infer,
 * the tensor of the last vp_infer_tensor / vp_detect_infer; AutoDrive: the pair vp_calibrate_range would run (an engine without VP_ACT_SCALE keeps no
 * previous frame: the resident frame is both halves) -- and, right behind the last launch that writes it, measures every tensor the plan stores in
 * HBM: abs-max and non-finite count of the stored value x = (float)hi + (float)lo (what vp_tensor_read returns; on a VP_ACT_SCALE engine
 * vp_tensor_read's value times 2^-exp), and a histogram of floor(log2 |x|) over the fp16 exponent range, 2^-24 (the smallest fp16 magnitude) up to
 * the top binade 2^15.  Exact zeros are counted apart, non-finite elements in neither; pad channels are not visited: count == c * h * w and
 * sum(bins) + zeros + nonfinite == count.  All counters are integer sums: two surveys of one input give equal words.
 *   out[i], i < min(cap, tensor count), belongs to tensor i of vp_tensor_info; tensors the plan never stores (views that only name a slice) keep
 *   count == 0 (exp is filled in for them too).  Returns the tensor count.  VP_ERR_ARG for a shared-prefix head or a batched encoder, VP_ERR_STATE when nothing is resident.  Never
 *   VP_ERR_RANGE: non-finite values are what it reports -- the first tensor in plan order with nonfinite > 0 is where a frame left the range.
 *   The engine is left as a plain pass over the same input leaves it (outputs on the device, fetched by vp_logits / vp_mask_u8 on use); no launch,
 *   exponent or graph changes, the next vp_infer replays the graph it replayed before.
 *   NOT seen: values that only live on chip -- the expanded tensor inside the fused MBConv kernels, the up-sampled tensor of a composed stage. */
#define VP_RANGE_BINS 40
#define VP_RANGE_EXP_MIN (-24)
typedef struct vp_range_stats {
  float absmax;                 /* of the stored value hi + lo, non-finite elements left out */
  int exp;                      /* VP_ACT_SCALE exponent of the tensor (true value = stored * 2^exp); 0 otherwise */
  unsigned long long count, nonfinite, zeros;
  unsigned long long bins[VP_RANGE_BINS];   /* bins[k]: floor(log2 |x|) == VP_RANGE_EXP_MIN + k */
} vp_range_stats;
int vp_range_survey(vp_engine* e, vp_range_stats* out, int cap);
/* RANGE GUARD.  Both precision modes compute on fp16 planes: VP_FP16X3 has fp32-class SIGNIFICAND (hi + lo) but fp16 EXPONENT range.
 *   - at load: a BN-folded weight with |w| > 65504 (or non-finite) fails vp_create* with VP_ERR_RANGE instead of loading as inf;
 *   - per frame: an activation beyond 65504 becomes inf and reaches the logits as inf / NaN; a probe kernel over the logits at the end
 *     of every pass (3 us, default ON) raises a flag that travels with the outputs, and the call that synchronises on that pass --
 *     vp_infer*, vp_fetch_outputs, vp_sync -- returns VP_ERR_RANGE (once per offending frame; the outputs of that frame are invalid).
 * The reference computes in fp32 and has no such limit; networks whose activations stay below 65504 (trained, normalised ones do by
 * orders of magnitude: |x| < 600 over the seeded sweeps of tests/test_gpu_parity_sweep.py) are unaffected.  enable = 0 drops the probe. */
int vp_set_finite_check(vp_engine* e, int enable);

/* ---- synchronous per-frame path (host buffers in, host buffers out) -------------------------------------- */
int vp_infer(vp_engine* e, const uint8_t* frame, int h, int w, int stride_bytes);
/* One frame through a base engine AND its shared-prefix heads (BASELINE metric: SceneSeg + Scene3D on one camera): one H2D,
 * all networks enqueued back to back on the base engine's stream, the selected outputs of every engine copied D2H behind
 * them, ONE host synchronisation -- instead of vp_infer + n x vp_infer_shared (n + 1 synchronisations). */
int vp_infer_multi(vp_engine* base, vp_engine* const* shared, int n_shared, const uint8_t* frame, int h, int w, int stride_bytes);
/* Asynchronous half of it for a frame that is already resident (vp_upload_frame): the base engine and its shared-prefix heads as
 * ONE graph launch on the base engine's stream.  Inside the graph the heads that consume only the backbone (Scene3D, EgoLanes on a
 * SceneSeg base) are forked behind it and joined at the end, so one frame's decoders overlap; results are bit-identical to
 * vp_enqueue(base) followed by vp_enqueue(head) for every head, and so is the stream order seen from outside. */
int vp_enqueue_multi(vp_engine* base, vp_engine* const* shared, int n_shared);
/* The fork is a LATENCY lever (measured on MI355X, SceneSeg + Scene3D: one camera 3.49 -> 3.19 ms per frame; three heads 4.47 ->
 * 3.99 ms) and a throughput loss when several cameras are already in flight on one GPU (three cameras: 390 -> 333 frames/s: the
 * chip is full, more concurrent kernels only contend).  Default 1 (the reference node is synchronous, one frame at a time);
 * a host that pipelines several cameras per GPU sets 0: vp_enqueue_multi / vp_infer_multi then enqueue one engine after the other. */
int vp_set_multi_fork(vp_engine* base, int enable);
int vp_infer_tensor(vp_engine* e, const float* nchw_1x3x320x640);
/* AutoDrive.forward(image_prev, image_curr) (autodrive_network.py:32-36): backbone on `prev`, then backbone + head on `curr`.
 * Plain vp_infer on a VP_AUTODRIVE engine is the streaming form: the previous call's frame is `prev` (the first frame of
 * a stream pairs with itself).  Both frames share h, w, stride. */
int vp_infer_pair(vp_engine* e, const uint8_t* prev, const uint8_t* curr, int h, int w, int stride_bytes);
int vp_logits(const vp_engine* e, const float** data, int64_t shape[4]);       /* host pointer, valid until next infer */
int vp_mask_u8(const vp_engine* e, const uint8_t** data, int* h, int* w);      /* host pointer, network resolution */
/* MasksVisualizationKernels::createMaskFromTensor{CUDA,HIP}(const float* host_tensor, shape, cv::Mat&) and
 * createEgoLanesMaskFromTensorCUDA (common/include/masks_visualization_kernels.hpp:14-45; Zenoh models/run_model.cpp): stateless,
 * HOST logits in, u8 mask out at tensor resolution, decode_mode as vp_decode_mode.  adapters/masks_visualization_kernels_hip.hpp
 * gives it the reference's exact signature (and skips the upload when the tensor is an engine's own logits). */
int vp_decode_logits_host(int gpu_id, const float* logits_nchw, int channels, int h, int w, int decode_mode, uint8_t* mask_out);
int vp_mask_resized_u8(vp_engine* e, uint8_t* dst, int h, int w);              /* nearest, to frame size */
int vp_depth_resized_f32(vp_engine* e, float* dst, int h, int w);              /* bilinear, plane 0 of the logits */
/* MasksVisualizationEngine::visualize (middleware_recipes/common/visualizers/masks_visualization_engine.cpp:11-58, SURVEY.md
 * 8f N4): colour LUT on the last mask (viz_type: 0 "scene", 1 "domain", 2 "egolanes" -- use VP_DECODE_LANE_LABEL for it),
 * nearest resize to the frame of the last vp_infer, 50/50 blend with that frame.  dst: BGR8 [frame_h][frame_w][3], packed. */
enum vp_viz_type { VP_VIZ_SCENE = 0, VP_VIZ_DOMAIN = 1, VP_VIZ_EGOLANES = 2 };
/* h, w: geometry of dst; VP_ERR_ARG unless it equals the last inferred frame's (the reference reads the size off original_image). */
int vp_visualize_mask_bgr8(vp_engine* e, int viz_type, uint8_t* dst_bgr8, int h, int w);
int vp_frame_hw(const vp_engine* e, int* h, int* w);                           /* geometry of the last uploaded frame */
/* DepthVisualizationEngine::visualize (middleware_recipes/common/visualizers/depth_visualization_engine.cpp:9-26): plane 0 of
 * the logits bilinear-resized to h x w (the map vp_depth_resized_f32 returns, run_model_node.cpp:100-104), min-max
 * normalised to u8 (convertTo with alpha = 255/(max-min), beta = -min*alpha; all zero if max == min) and mapped through
 * COLORMAP_VIRIDIS.  dst: BGR8 [h][w][3], packed.  Table and convertTo rounding restated from published sources, not
 * pinned against OpenCV (absent here) -- see DESIGN.md. */
int vp_visualize_depth_bgr8(vp_engine* e, uint8_t* dst_bgr8, int h, int w);
int vp_input_tensor(vp_engine* e, float* dst_1x3x320x640);                     /* the post-resize network input */

/* ---- AutoSteer hand-over (VisionPilot/production_release/main.cpp:472-534) ---------------------------
 * The production app feeds its AutoSteer head the raw EgoLanes logits of the last TWO frames, concatenated [t-1 | t] = fp32 {1, 6, 80, 160}:
 * a boost::circular_buffer of host copies plus two memcpys per frame (main.cpp:508-530), handed to AutoSteerOnnxEngine::inference
 * (src/inference/autosteer_engine.cpp:104-195).  With vp_set_lane_ring(e, 1) a VP_EGOLANES engine keeps that buffer ON THE DEVICE: two
 * device-to-device copies behind every pass (inside the replayed graph), no host round trip -- a device-resident AutoSteer runtime reads
 * vp_lane_ring_device, the reference's host-side engine reads vp_lane_ring_fetch.  *frames_valid = passes since enabling, capped at 2: the
 * reference runs AutoSteer only once two frames are in (main.cpp:521).  The AutoSteer GRAPH itself is not in the reference tree (ONNX only,
 * production_release/README.md:112): the head is not built, its input is.  VP_ERR_ARG on other model kinds, VP_ERR_STATE while disabled. */
int vp_set_lane_ring(vp_engine* e, int enable);
int vp_lane_ring_device(const vp_engine* e, void** dev_f32_6x80x160, int* frames_valid);
int vp_lane_ring_fetch(vp_engine* e, float* dst_host_6x80x160, int* frames_valid);
/* The other end of that head, AutoSteerOnnxEngine::postProcess (autosteer_engine.cpp:160-185): arg-max over the `classes` (61) logits of the head's
 * SECOND output, strict '>' from class 0 (the first maximum wins, a NaN never wins), steering angle = class - 30 degrees.  Host arithmetic on 61 floats
 * (no device work): offered so that a host replacing the engine class keeps the decode bit for bit.  Returns 0 (the reference's failure value) for
 * logits == NULL or classes < 1. */
float vp_autosteer_angle(const float* logits, int classes);

/* ---- asynchronous / device-resident path (bench, multi-GPU) ---------------------------------------------- */
int vp_upload_frame(vp_engine* e, const uint8_t* frame, int h, int w, int stride_bytes); /* H2D, frame stays in HBM */
int vp_enqueue(vp_engine* e);                                                  /* one pass over the resident frame */
int vp_sync(vp_engine* e);
int vp_fetch_outputs(vp_engine* e);                                            /* D2H logits + mask, then sync */
int vp_device_outputs(const vp_engine* e, void** logits_f32, void** mask_u8);  /* device pointers (D2D gathers) */
int vp_copy_outputs_device(vp_engine* e, void* logits_dst, void* mask_dst);   /* async D2D on the engine stream */
int vp_use_graph(vp_engine* e, int enable);                                    /* hipGraph replay (default on) */
int vp_timer_begin(vp_engine* e);                                              /* hipEvent on the engine stream */
int vp_timer_end(vp_engine* e, float* elapsed_ms);                             /* records, syncs, returns elapsed */

/* ---- vp_frame: one camera frame, uploaded once in its native format, for every engine ------------------------------------------
 * The reference's production application (VisionPilot/production_release/main.cpp) feeds ONE captured frame to a lateral thread (EgoLanes on the
 * crop rows >= 420, main.cpp:497-505) and a longitudinal thread (AutoSpeed), and its sensor path converts to BGR on the CPU first
 * (common/sensors/gstreamer_engine.cpp:33-47 `videoconvert ! video/x-raw,format=BGR`; run_model_node.cpp:70 toCvCopy(BGR8)) although V4L2 cameras and
 * hardware decoders deliver YUY2 / UYVY / NV12.  With vp_infer / vp_detect_infer every network pays its own staging copy and its own H2D for the
 * same bytes.  A vp_frame takes the frame ONCE, in the format it arrives in, converts it on the device to BGR8 and hands regions of it to any number
 * of consumers:
 *     vp_frame_upload(f, VP_FRAME_YUY2, &data, &stride, 1, 720, 1280);
 *     thread A: vp_infer_frame(egolanes, f, 0, 420, 1280, 300);      thread B: vp_detect_infer_frame(det, f, 0, 0, 0, 0, ...);
 * A vp_frame always holds packed BGR8.  BGR8 is copied straight in; RGB8 / BGRA8 / RGBA8 are permuted or lose alpha; GRAY8 is replicated to three
 * channels; the YUV formats use, by default, the integer BT.601 limited-range form OpenCV documents for cvtColor(COLOR_YUV2BGR_NV12 / _YUY2 / _UYVY):
 * 20-bit fixed point, no chroma interpolation (NV12 / NV21 / I420 / YV12 share one (U, V) per 2x2 block, YUY2 = Y0 U Y1 V and UYVY = U Y0 V Y1 one per
 * horizontal pixel pair):
 *     y = 1220542 * max(0, Y - 16);  u = U - 128;  v = V - 128
 *     R = sat8((y + 1673527 * v               + (1 << 19)) >> 20)
 *     G = sat8((y -  852492 * v - 409993 * u  + (1 << 19)) >> 20)
 *     B = sat8((y + 2116026 * u               + (1 << 19)) >> 20)         arithmetic shift, then clamp to 0 .. 255
 * This formula IS the definition; parity with OpenCV itself is not pinned (OpenCV is absent here: DESIGN.md section 4).
 * COLOUR STANDARD.  vp_frame_set_color(f, matrix, range) chooses the constants of LATER uploads of the YUV formats (the picture a frame already holds
 * stays as its upload made it); the default (VP_COLOR_BT601, VP_COLOR_RANGE_LIMITED) is the formula above, to the bit.  The form never changes:
 *     y = CY * max(0, Y - off);  u = U - 128;  v = V - 128
 *     R = sat8((y + CVR v + (1 << 19)) >> 20);  G = sat8((y - CVG v - CUG u + (1 << 19)) >> 20);  B = sat8((y + CUB u + (1 << 19)) >> 20)
 *                        off       CY      CVR      CVG      CUG      CUB
 *     BT.601 limited      16  1220542  1673527   852492   409993  2116026     OpenCV's constants, kept as they are
 *     BT.601 full          0  1048576  1470104   748826   360853  1858077
 *     BT.709 limited      16  1220945  1879825   558796   223607  2215014
 *     BT.709 full          0  1048576  1651297   490864   196424  1945738
 * The three new rows are exact: each constant is the nearest integer to coefficient x 2^20, the coefficients derived from (Kr, Kb) = (0.299, 0.114) /
 * (0.2126, 0.0722) as rationals, scaled by 255/219 (luma) and 255/224 (chroma) in limited range and by 1 in full range.  |y + chroma| < 2^30 for every
 * byte input.  Black is (off, 128, 128), white (235 or 255, 128, 128).  Like the default they ARE the definition and are not pinned against OpenCV.
 * HD cameras and hardware decoders deliver BT.709; MJPEG cameras and every JPEG-derived stream are full range (BT.601 full).  The settings do not touch
 * BGR8 / RGB8 / BGRA8 / RGBA8 / GRAY8 uploads.  VP_ERR_ARG (with text) for an unknown matrix or range; a refused call changes nothing.
 * planes / strides, in bytes: 1 plane; 2 for NV12 (Y, then interleaved U V) and NV21 (Y, then interleaved V U: rows of w bytes, h / 2 of them); 3 for
 * I420 (Y, U, V) and YV12 (Y, V, U): chroma planes of h / 2 rows of w / 2 bytes.  One (U, V) per 2x2 block in all four.  VP_ERR_ARG (with text): odd w
 * for NV12 / YUY2 / UYVY / I420 / YV12 / NV21, odd h for NV12 / I420 / YV12 / NV21, h or w below 2, a stride below the row's bytes, a wrong n_planes, an
 * unknown format (codes 8 .. 15 are not used).
 * vp_frame_upload is ASYNCHRONOUS on the frame's own stream.  Host planes are staged through the frame's pinned double buffer (copied before the call
 * returns) or, when every plane lies inside a vp_register_frames range, copied by one DMA per plane straight from the caller's memory -- the rules
 * of vp_upload_frame, including that such planes stay unmodified until vp_frame_sync or a consumer's synchronising call.
 * vp_frame_upload_device takes the planes from DEVICE memory on the frame's GPU (a decoder surface, another HIP producer) and converts straight from
 * them (no intermediate copy): they must stay valid and unmodified until the conversion has run (vp_frame_sync, or any consumer's synchronising
 * call).  producer_stream: a hipStream_t the planes are ready on -- the frame's stream waits for the work queued on it so far -- or NULL = ready now
 * (NULL also spells HIP's legacy default stream, which therefore cannot be named: synchronise it first, or produce on a created stream).
 * ORDERING CONTRACT.  Consumers never wait on the host for the frame: the consumer's stream waits (hipStreamWaitEvent) for the frame's "content
 * ready" event.  A later vp_frame_upload* orders itself ON THE DEVICE behind every consumer copy queued so far (each consumer records an event behind
 * its copy; the frame waits for them in its own stream), so the host may re-upload without synchronising anything:
 *     upload(A); vp_upload_from_frame(e1, f, ..); vp_enqueue(e1); upload(B); vp_upload_from_frame(e2, f, ..); vp_enqueue(e2);   e1 sees A, e2 sees B.
 * THREADING.  One thread uploads; any number of threads consume concurrently, each on its own engine / detector.  An upload CONCURRENT with a
 * consumer call on the same vp_frame is the host's race to avoid: use two frames, ping-pong, as the reference's DoubleFrameBuffer does
 * (INTEGRATION.md "One camera frame, several networks").  A frame must outlive the passes that consume it.  No process-wide state.
 *
 * RAW BAYER, P010 AND 16-BIT GREY (upload only: vp_frame_upload / vp_frame_upload_device take them, vp_canvas_fetch* and vp_canvas_layout* refuse them
 * as unknown formats).  GMSL / MIPI sensors deliver raw Bayer, 8 bits or 10 / 12 bits in 16-bit words; HEVC Main10 and AV1 10-bit decoders deliver P010
 * surfaces; thermal and mono sensors 16-bit grey.  16-bit samples are little-endian words.
 *   VP_FRAME_BAYER_<order>8 / _<order>16: 1 plane, rows of w bytes / 2 w bytes.  The four letters name the 2x2 cell at (row 0, column 0) in reading
 *     order: RGGB means row 0 is R G and row 1 is G B.
 *   VP_FRAME_P010: 2 planes; plane 0 holds Y as 16-bit words in rows of 2 w bytes, plane 1 interleaved U V words in rows of 2 w bytes, h / 2 rows.
 *   VP_FRAME_GRAY16: 1 plane, rows of 2 w bytes.
 * VP_ERR_ARG (with text; a refused call changes nothing): odd w or h for P010 and every Bayer format, h or w below 2, a stride below the row's bytes, a
 * wrong n_planes, for the 16-bit formats an odd stride or an odd plane address, a raw setting that does not fit the format (below).
 * P010 and GRAY16 narrow every 16-bit sample first, x8 = min(255, (s + 128) >> 8) (samples are MSB-aligned, as P010, P012 and P016 all are); P010 is
 * then NV12's arithmetic on (Y8, U8, V8) to the bit, the colour standard of vp_frame_set_color included, and GRAY16 is GRAY8's on the narrowed sample.
 * (A full 10-bit matrix form would overflow the 32-bit form the YUV definition rests on; narrowing first keeps ONE definition.)
 * THE RAW DEFINITION.  vp_frame_set_raw(f, &r) holds for LATER uploads of the Bayer formats and touches no other format.  Let B be the significant
 * bits (r.bits, or with r.bits = 0 the container's width, 8 or 16) and M = 2^B - 1.  Every sample s is processed by the colour c of its CFA site, all
 * in 32-bit integer arithmetic:
 *   1. linearise       v = max(0, min(s >> shift, M) - black)
 *   2. white balance   v = min(M, (v * gains[c] + 128) >> 8)                    gains in Q8, order R, G, B
 *   3. bilinear demosaic at B bits: at a site of colour c, channel c is v; at an R or B site, G = (N + S + W + E + 2) >> 2 and the opposite colour is
 *      (NW + NE + SW + SE + 2) >> 2; at a G site, the colour of its horizontal neighbours is (W + E + 1) >> 1 and the other colour (N + S + 1) >> 1.
 *      Borders mirror without repeating the edge, index -1 -> 1 and n -> n - 2: CFA parity is kept, so every average takes same-colour samples only.
 *   4. optional matrix o_i = clamp((sum_j ccm[3 i + j] * x_j + 512) >> 10, 0, M)     Q10, rows and columns in R, G, B order
 *   5. tone            with a LUT: out8 = lut[x >> (B - min(B, 12))];  without: out8 = x for B = 8, else min(255, (x + (1 << (B - 9))) >> (B - 8))
 *   6. store B, G, R.
 * 65535 * 16383 + 128 < 2^31 and 3 * 8191 * 65535 + 512 < 2^31, so nothing overflows.  This IS the definition (tests/raw_cases.py restates it in numpy);
 * like every sibling conversion it is not pinned against OpenCV.  A picture that is constant per channel comes back exact at every pixel, borders
 * included.
 * vp_raw defaults (vp_frame_set_raw(f, NULL)): bits 0, shift 0, black 0, gains {256, 256, 256}, ccm_on 0, no LUT.  The LUT is copied at the call.
 * VP_ERR_ARG at set (nothing changes): bits not in {0, 8, 10, 12, 14, 16}, shift outside 0 .. 8, black < 0, a gain outside 0 .. 16383, ccm_on with any
 * |ccm[i]| > 8191, lut without lut_len or lut_len without lut, lut_len not in {256, 1024, 4096}.  VP_ERR_ARG at the upload, where B is known: bits == 8
 * with a 16-bit format, bits > 8 with an 8-bit format, black > M, lut_len != 2^min(B, 12). */
typedef struct vp_frame vp_frame;
enum vp_frame_format { VP_FRAME_BGR8 = 0, VP_FRAME_RGB8 = 1, VP_FRAME_BGRA8 = 2, VP_FRAME_RGBA8 = 3, VP_FRAME_GRAY8 = 4,
                       VP_FRAME_NV12 = 5, VP_FRAME_YUY2 = 6, VP_FRAME_UYVY = 7, VP_FRAME_I420 = 16, VP_FRAME_YV12 = 17, VP_FRAME_NV21 = 18,
                       VP_FRAME_GRAY16 = 20, VP_FRAME_P010 = 21,      /* 8 .. 15 and 19 are not used */
                       VP_FRAME_BAYER_RGGB8 = 32, VP_FRAME_BAYER_GRBG8 = 33, VP_FRAME_BAYER_GBRG8 = 34, VP_FRAME_BAYER_BGGR8 = 35,
                       VP_FRAME_BAYER_RGGB16 = 36, VP_FRAME_BAYER_GRBG16 = 37, VP_FRAME_BAYER_GBRG16 = 38, VP_FRAME_BAYER_BGGR16 = 39 };
typedef struct vp_raw { int bits, shift, black; int gains[3]; int ccm_on; int ccm[9]; const uint8_t* lut; int lut_len; } vp_raw;
enum vp_color_matrix { VP_COLOR_BT601 = 0, VP_COLOR_BT709 = 1 };
enum vp_color_range { VP_COLOR_RANGE_LIMITED = 0, VP_COLOR_RANGE_FULL = 1 };
enum vp_chroma_mode { VP_CHROMA_EVEN = 0, VP_CHROMA_MEAN = 1 };
int vp_frame_create(vp_frame** out, int gpu_id, char* err, size_t err_len);
void vp_frame_destroy(vp_frame* f);
const char* vp_frame_last_error(const vp_frame* f);
int vp_frame_upload(vp_frame* f, int format, const uint8_t* const* planes, const int* strides, int n_planes, int h, int w);
int vp_frame_upload_device(vp_frame* f, int format, const void* const* dev_planes, const int* strides, int n_planes, int h, int w, void* producer_stream);
int vp_frame_set_color(vp_frame* f, int matrix, int range);              /* applies to later uploads */
int vp_frame_get_color(const vp_frame* f, int* matrix, int* range);
int vp_frame_set_raw(vp_frame* f, const vp_raw* r);                      /* NULL: defaults; applies to LATER uploads of the Bayer formats, like vp_frame_set_color */
int vp_frame_get_raw(const vp_frame* f, vp_raw* out);                    /* lut comes back NULL; lut_len tells whether one is installed */
int vp_frame_sync(vp_frame* f);                                          /* waits for the frame's own stream (upload + conversion) */
int vp_frame_dims(const vp_frame* f, int* h, int* w);                    /* geometry of the last upload; VP_ERR_STATE before it (vp_frame_hw is the engine's) */
int vp_frame_fetch_bgr8(vp_frame* f, uint8_t* dst, int dst_stride);      /* the converted image, synchronous (tests, hosts that still want a cv::Mat) */
/* Consumers.  vp_upload_from_frame is the asynchronous twin of vp_upload_frame: the engine's stream waits for the frame's content, then copies the
 * region (x0, y0, w, h; all four 0: the whole frame) device to device, rows packed, into the engine's own frame buffer -- from there on the pass is
 * vp_enqueue / vp_sync / vp_fetch_outputs as today, and everything behind the upload is the host path's: tap tables, a geometry change leading to
 * graph re-capture, vp_visualize_mask_bgr8's "last frame", AutoDrive's streaming pair.  A region gives the bits vp_upload_frame gives for the same
 * pixels passed as a strided view.  vp_infer_frame = that + what vp_infer does behind its upload.  vp_detect_infer_frame = vp_detect_infer on the
 * region (VP_AUTOSPEED engine attached).
 * Accepted: the scene kinds, VP_AUTODRIVE (streaming form), VP_AUTOSTEER (the region must be 512 x 1024).  VP_ERR_ARG: a shared-prefix head (frames
 * go to the base), a batched encoder, an engine whose vp_set_input_format pixel format is not VP_BGR8, a frame on another GPU, a region outside the
 * frame or smaller than 2 x 2; a VP_AUTOSPEED engine: the refusal vp_upload_frame gives; a frame never uploaded: VP_ERR_STATE. */
int vp_upload_from_frame(vp_engine* e, vp_frame* f, int x0, int y0, int w, int h);
int vp_infer_frame(vp_engine* e, vp_frame* f, int x0, int y0, int w, int h);

/* ---- vp_frame rectification: undistort and warp to the standard camera pose, on the device ---------------------------------------
 * The reference's Camera Calibration Protocol (VisionPilot/calibration/README.md, calibration.py, demo.py) puts every deployed camera's frame through
 *     cv2.undistort(frame, K, dist)                                                                          (calibration.py:52-81)
 *     cv2.warpPerspective(frame, K_s_mod . R_rel . K_i^-1, (w_s, h_s), borderMode = BORDER_REPLICATE)         (calibration.py:170-204)
 * before any network sees it (standard pose: 1024 x 512).  vp_frame_set_rectify makes LATER uploads do both on the device, on the frame's own stream,
 * behind the format conversion and ahead of the "content ready" event: from there on the frame IS the standard-pose picture -- vp_frame_dims answers
 * (out_h, out_w), vp_frame_fetch_bgr8, every region consumer and vp_canvas_begin see it, and detections, masks and lane rows come out in
 * standard-pose coordinates.  The ordering contract above is unchanged.  NULL switches rectification off; without the setting an upload runs exactly
 * the launches and gives exactly the bits it did before the setting existed.
 * The formulas below ARE the definition.  OpenCV is absent here, so parity with cv2.undistort / cv2.warpPerspective is not pinned (as for cv::resize
 * and cvtColor).
 * SAMPLE.  A map entry of a destination pixel is (X, Y): the source coordinates in units of 1/32 pixel, integers.
 *     ix = X >> 5, iy = Y >> 5 (arithmetic shift);  fx = X & 31, fy = Y & 31
 *     taps     (ix, iy)            (ix + 1, iy)      (ix, iy + 1)      (ix + 1, iy + 1)
 *     weights  (32 - fx)(32 - fy)  fx (32 - fy)      (32 - fx) fy      fx fy                     sum 1024
 *     out = (sum of weight x byte + 512) >> 10                                                  per channel
 *   (the familiar 32 x 32 table of 15-bit weights with + 2^14 >> 15 gives the same value: every weight times 32 is an integer).
 *   VP_BORDER_CONSTANT: a tap outside the source contributes 0.  VP_BORDER_REPLICATE: tap coordinates are clamped to the picture.
 * COORDINATES are computed in IEEE double, in the order written, with no fused multiply-add.  X = rne(32 u): round half to even, then clamp to
 *   [-2^20, 2^20 - 1] (a NaN takes the lower clamp).  They are exchanged as int16 (ix, iy) pairs plus uint16 frac = fy << 5 | fx.
 * UNDISTORT MAP.  Destination size = source size.  K = [fx 0 cx; 0 fy cy; 0 0 1], dist = (k1, k2, p1, p2, k3) (OpenCV's order).  For pixel (j, i):
 *     x = (j - cx) / fx;  y = (i - cy) / fy;  r2 = x x + y y
 *     kr = 1 + ((k3 r2 + k2) r2 + k1) r2
 *     xd = x kr + p1 (2 (x y)) + p2 (r2 + 2 (x x))
 *     yd = y kr + p1 (r2 + 2 (y y)) + p2 (2 (x y))
 *     u = fx xd + cx;  v = fy yd + cy                        X = rne(32 u), Y = rne(32 v);  border CONSTANT (value 0), as cv2.undistort
 * PERSPECTIVE MAP.  Destination out_w x out_h; H maps source to destination, as cv2.warpPerspective takes it.  M = adj(H) / det(H) with
 *     a0 = H4 H8 - H5 H7   a1 = H2 H7 - H1 H8   a2 = H1 H5 - H2 H4
 *     a3 = H5 H6 - H3 H8   a4 = H0 H8 - H2 H6   a5 = H2 H3 - H0 H5
 *     a6 = H3 H7 - H4 H6   a7 = H1 H6 - H0 H7   a8 = H0 H4 - H1 H3        det = (H0 a0 + H1 a3) + H2 a6;   Mi = ai / det
 *   For destination (x, y):  X0 = (M0 x + M1 y) + M2;  Y0 = (M3 x + M4 y) + M5;  W = (M6 x + M7 y) + M8;  s = W != 0 ? 32 / W : 0
 *     X = rne(clamp(X0 s, -2^31, 2^31)), Y likewise, then the clamp to [-2^20, 2^20 - 1];  border REPLICATE.
 * MODES.  VP_RECTIFY_TWO_PASS (default) is the protocol's own pipeline: pass 1 undistort, raw -> raw-sized; pass 2 warp, raw-sized -> out.  A pass whose
 *   map is the identity is skipped, which is exact (frac = 0: (1024 p + 512) >> 10 = p): pass 1 when all five coefficients are 0, pass 2 when H is the
 *   identity and out equals the raw size.
 *   VP_RECTIFY_ONE_PASS (opt-in): ONE map, one resampling.  For destination (x, y): (px, py) = (W != 0 ? X0 / W : 0, likewise Y0) clamped to
 *   [0, w - 1] x [0, h - 1] (REPLICATE on the undistorted domain); then the distortion formulas with x = (px - cx) / fx, y = (py - cy) / fy;
 *   X = rne(32 u), Y = rne(32 v); border CONSTANT on the raw picture.  Half the traffic and one interpolation instead of two -- and therefore NOT bit-equal
 *   to the two passes (DESIGN.md records the difference on a smooth picture).
 * COST.  The maps are built on the host (the code behind vp_rectify_map), uploaded and kept per raw geometry (src_h, src_w); they are rebuilt only when
 *   the geometry or the setting changes: one host computation and one host wait per geometry, next to the one of a growing buffer.
 * REFUSALS (VP_ERR_ARG with text; a refused call changes nothing): a non-finite value; fx or fy equal to 0; K[1], K[3], K[6], K[7] not 0 or K[8] not 1
 *   (no skew); det H = 0 (or not finite); out_w / out_h outside 2 .. 16384; an unknown mode.
 * vp_rectify_map (host only, no device): the map `which` (0 undistort, 1 warp, 2 one-pass) for a src_h x src_w source in the exchange form: xy
 *   [n][2] int16 (ix, iy), frac [n] uint16, n = src_h * src_w (which 0) or out_h * out_w, row-major.
 * vp_rectify_homography (host only) restates calibration.py:16-49, 84-204: R = Rodrigues of the vector (pitch, yaw, roll) in radians (identity at
 *   angle 0); R_rel = R_s . R_i^-1 (the inverse of a rotation: its transpose);  f_s = (w_s / 2) / tan(hfov_s / 2), K_s = [f_s 0 w_s/2; 0 f_s h_s/2; 0 0 1];
 *   K_s_mod = K_s with its [1][1] multiplied by camera_height_s / camera_height_i;  H = K_s_mod . R_rel . K_i^-1.  Of `inference` it reads the angles,
 *   camera_height and K; of `standard` the angles, camera_height, img_w, img_h and hfov_deg.  VP_ERR_ARG: a non-finite value, a zero camera_height of
 *   the inference pose, fx or fy of K 0 or K skewed, img_w / img_h below 1, hfov outside (0, 180). */
enum vp_rectify_mode { VP_RECTIFY_TWO_PASS = 0, VP_RECTIFY_ONE_PASS = 1 };
enum vp_border { VP_BORDER_CONSTANT = 0, VP_BORDER_REPLICATE = 1 };
typedef struct vp_rectify {
  double K[9];
  double dist[5];
  double H[9];
  int out_w, out_h;
  int mode;
} vp_rectify;
int vp_frame_set_rectify(vp_frame* f, const vp_rectify* r);              /* NULL: off; applies to LATER uploads, like vp_frame_set_color */
int vp_frame_get_rectify(const vp_frame* f, vp_rectify* out);            /* VP_ERR_STATE when off */
int vp_rectify_map(const vp_rectify* r, int src_h, int src_w, int which, int16_t* xy, uint16_t* frac);
typedef struct vp_camera_pose {
  double pitch_deg, yaw_deg, roll_deg, camera_height;
  double K[9];
  int img_w, img_h;
  double hfov_deg;
} vp_camera_pose;
int vp_rectify_homography(const vp_camera_pose* inference, const vp_camera_pose* standard, double H_out[9]);

/* ---- vp_canvas: one picture per camera frame, composed on the device, fetched once in any vp_frame format -------------------------
 * The output side of vp_frame.  MasksVisualizationEngine / DepthVisualizationEngine / AutoSpeedVisualizationEngine each take the host frame and return
 * one host picture per network (the ROS2 README times the step at 25 ms per frame); vp_visualize_mask_bgr8 / vp_visualize_depth_bgr8 above are their
 * device twins: one overlay, one host synchronisation and one full-frame D2H per call, base engines only, each blending with its own crop.  A vp_canvas
 * is ONE picture of the camera frame that every engine -- of any scene kind, shared-prefix heads included -- and the detector draw into on the device:
 *     vp_canvas_begin(c, f);                                  the canvas becomes a copy of the frame's BGR8 picture (device to device)
 *     vp_canvas_blend_mask(c, sceneseg, VP_VIZ_SCENE);        each engine draws into the region its input came from
 *     vp_canvas_paste_depth(c, scene3d_head);  vp_canvas_blend_mask(c, egolanes, VP_VIZ_EGOLANES);  vp_canvas_draw_detections(c, dets, n);
 *     vp_canvas_fetch(c, VP_FRAME_NV12, planes, strides, 2);  one synchronisation, one D2H, in the format the encoder / display wants
 * WHERE AN ENGINE DRAWS.  An engine records where its resident input came from: vp_upload_from_frame / vp_infer_frame record the region (x0, y0, w, h)
 * and the source frame's (H, W); the host uploads (vp_upload_frame*, vp_infer*) record the whole frame, (0, 0, w, h) of (h, w); a shared-prefix head
 * uses its base's record.  vp_canvas_blend_mask / vp_canvas_paste_depth return VP_ERR_ARG when the recorded (H, W) is not the canvas's geometry (the
 * text names both), for an engine on another GPU, a tensor-input engine, a batched encoder and the VP_AUTODRIVE / VP_AUTOSPEED / VP_AUTOSTEER kinds (no
 * mask or depth plane); VP_ERR_STATE ("Inference has not been run yet") before the engine's first pass, and on a canvas without a picture.
 * vp_canvas_begin: the picture, geometry and row pitch (12 * ceil(w / 4) bytes) of the frame; the copy runs on the canvas's own stream behind the
 *   frame's "content ready" event and counts as a consumer of the frame: a later vp_frame_upload* orders itself behind it on the device.  VP_ERR_STATE
 *   for a frame never uploaded, VP_ERR_ARG for a frame on another GPU.  A second begin discards the picture and may change the geometry.
 * vp_canvas_blend_mask: viz_type as vp_visualize_mask_bgr8 (VP_VIZ_EGOLANES wants VP_DECODE_LANE_LABEL, as there).  The engine's last mask is
 *   nearest-resized to the region (the index rule of vp_mask_resized_u8, tables of the region's h and w), coloured through the same table and blended
 *   50 / 50 with the canvas pixels of the region, in place: (a + b) >> 1, odd sums to even.  Pixels outside the region are untouched.  EXACT against
 *   the existing call: on a fresh canvas the region's bytes equal vp_visualize_mask_bgr8 of a base engine that took that region.
 * vp_canvas_blend_mask_u8: the operator entry -- the same for a caller's mh x mw u8 label mask (host, or device memory on the canvas's GPU that is
 *   complete when the call is made) into an explicit region.  VP_ERR_ARG: a region outside the canvas or smaller than 2 x 2, mh or mw < 1.  A host
 *   mask is copied before the call returns.
 * vp_canvas_paste_depth: plane 0 of the engine's logits through the pipeline of vp_visualize_depth_bgr8(e, dst, region h, region w) -- bilinear resize
 *   to the region's size, min-max, the same rounding, the same table -- written opaquely into the region.  EXACT: the region's bytes equal that call's.
 * vp_canvas_draw_detections: AutoSpeedVisualizationEngine::drawUntrackedDetection (autospeed_visualization_engine.cpp:126-140) without its text.  For
 *   each detection in order: bx = (int)x1, by = (int)y1, bw = (int)(x2 - x1), bh = (int)(y2 - y1) (float subtraction, truncation toward zero); nothing
 *   if bw <= 0 or bh <= 0; the inclusive rectangle [bx, bx + bw - 1] x [by, by + bh - 1], clipped to the canvas, gets the 20 % fill
 *   d = nearest integer to (colour + 4 d) / 5 per channel (never a tie: the fraction is a multiple of 0.2; both float32 spellings of
 *   addWeighted(overlay, 0.2, frame, 0.8) give it), then the rectangle's one-pixel outline is set to the colour -- the outline of the rectangle BEFORE
 *   clipping, as cv::rectangle draws it: a side that lies outside the canvas is not drawn, the box stays open there.  Colours by class_id, BGR:
 *   1 (0, 0, 255), 2 (0, 255, 255), 3 (255, 255, 0), anything else white.  Later boxes draw over earlier ones.  n = 0: nothing; VP_ERR_ARG for
 *   n < 0, null with n > 0, a non-finite or absurd (|v| >= 1e8) coordinate.  This rule IS the definition; it is not pinned against OpenCV (absent
 *   here, as for the other OpenCV restatements: DESIGN.md section 4).  Text, the tracked-object style, the CIPO tag and the warnings are not built.
 * vp_canvas_fetch: synchronous; every vp_frame_format.  BGR8 as it is; RGB8 / BGRA8 / RGBA8 permuted, alpha 255; GRAY8 and the YUV formats by the
 *   FORWARD form, the integer counterpart of the upload formula above (20 fractional bits, arithmetic shift, clamp 0 .. 255); by default BT.601
 *   limited range:
 *     Y = ( 269484 R + 528482 G + 102760 B + (16  << 20) + (1 << 19)) >> 20
 *     U = (-155188 R - 305135 G + 460324 B + (128 << 20) + (1 << 19)) >> 20
 *     V = ( 460324 R - 385875 G -  74448 B + (128 << 20) + (1 << 19)) >> 20
 *   GRAY8 is Y; chroma is taken from the EVEN pixel of a pair (the 2x2 formats: the top-left pixel of the block), no averaging.  Black gives
 *   (16, 128, 128), white (235, 128, 128), pure red V = 240.  This formula IS the definition; it is not pinned against OpenCV.
 *   vp_canvas_set_color(c, matrix, range, chroma_mode) chooses the standard and the chroma rule of LATER fetches; it outlives vp_canvas_begin.  A canvas
 *   does NOT inherit the standard of the frame it was begun on: a host that wants the camera's standard back sets it here as well.  The default
 *   (VP_COLOR_BT601, VP_COLOR_RANGE_LIMITED, VP_CHROMA_EVEN) is the formula above, to the bit.  In general
 *     Y = (YR R + YG G + YB B + (off << 20) + (1 << 19)) >> 20;   U, V likewise with (128 << 20) in place of the offset
 *                        off       YR      YG      YB        UR       UG      UB       VR       VG      VB
 *     BT.601 limited      16   269484  528482  102760   -155188  -305135  460324   460324  -385875  -74448
 *     BT.601 full          0   313524  615514  119538   -176932  -347356  524288   524288  -439026  -85262
 *     BT.709 limited      16   191455  644067   65019   -105533  -355018  460551   460551  -418321  -42230
 *     BT.709 full          0   222927  749942   75707   -120138  -404150  524288   524288  -476214  -48074
 *   The three new rows are the nearest integers to coefficient x 2^20 (derived as for the upload), except UB and VR, which are minus the sum of their
 *   row's other two constants, so that grey gives exactly (128, 128).  |pre-shift| < 2^30 for every byte input.  In full range pure blue (U) and pure
 *   red (V) reach 256 before the clamp: there the clamp decides.  GRAY8 is the Y of the chosen standard; the RGB family is untouched.
 *   VP_CHROMA_MEAN: U and V are first formed per pixel as clamped bytes by the forward formula; a 2x2 group (NV12 / NV21 / I420 / YV12) then stores
 *   (a + b + c + d + 2) >> 2, a 2x1 pair (YUY2 / UYVY) (a + b + 1) >> 1.  VP_CHROMA_EVEN is the rule above.  (Upload has no counterpart: no chroma
 *   interpolation there.)  VP_ERR_ARG (with text) for an unknown matrix, range or chroma mode.
 *   Refusals as vp_frame_upload: odd w for the YUV formats, odd h for NV12 / I420 / YV12 / NV21, a stride below the row's bytes, a wrong n_planes, an
 *   unknown format.  vp_canvas_layout3 (host only, no device) answers the planes of (format, h, w): n_planes, bytes per row and rows of each;
 *   VP_ERR_ARG for the same geometry refusals.  vp_canvas_layout is the same with room for two planes: VP_ERR_ARG for I420 / YV12.
 * THE PRODUCTION DISPLAY (production_release/main.cpp:881-907: boxes, lanes by drawRawMasksInPlace, cv::resize to 1280 x 720) as calls:
 *     vp_canvas_begin(c, f);  vp_canvas_draw_detections(c, dets, n);  vp_canvas_overlay_lanes(c, egolanes, 0.0f);
 *     vp_canvas_fetch_resized(c, VP_FRAME_NV12, 720, 1280, planes, strides, 2);
 * vp_canvas_add_planes_f32: the operator entry of the additive overlay.  planes: fp32 [n_planes][mh][mw] -- host memory, copied before the call returns,
 *   or (planes_on_device) device memory on the canvas's GPU that is complete when the call is made; add_bgr: u8 [n_planes][3], host.  For every canvas
 *   pixel of the region (x0, y0, w, h), (my, mx) comes from the nearest tables of vp_mask_resized_u8 (the region's h and w into mh and mw, as
 *   vp_canvas_blend_mask_u8); every plane k with planes[k][my][mx] > threshold (fp32 compare: NaN is false) adds add_bgr[k] to the pixel, and each
 *   channel becomes min(255, d + the sum of those increments).  All increments are non-negative, so the one clamped sum equals the overlays applied one
 *   after the other in any order; a pixel that belongs to two planes shows both.  VP_ERR_ARG: n_planes outside 1 .. 4, a null pointer, mh or mw
 *   outside 1 .. 16384, a threshold that is not finite, a region outside the canvas or smaller than 2 x 2.  VP_ERR_STATE on a canvas without a picture.
 * vp_canvas_overlay_lanes: drawRawMasksInPlace (production_release/src/visualization/visualize.cpp:312-388) on a VP_EGOLANES engine (base or
 *   shared-prefix head): the engine's device logits {1, 3, 80, 160} are the planes -- 0 ego left, 1 ego right, 2 other lanes -- drawn into the region
 *   the engine's input came from.  The reference makes three overlays addWeighted(image, 1.0, colour layer under the mask, 0.4) with the BGR colours
 *   (0, 153, 0) other, (255, 0, 0) ego left, (255, 0, 200) ego right: on a byte d that is d + 0.4 colour rounded, the same increment for every d and
 *   never a tie in either float32 spelling of addWeighted -- other (0, 61, 0), ego left (102, 0, 0), ego right (102, 0, 80) -- then the clamp to 255.
 *   `threshold` is compared with the raw logit (the reference thresholds its own post-processed planes: the caller chooses the value that corresponds).
 *   Any decode mode: only the logits are read.  The reference overlays on a 640 x 320 copy of the region and resizes that copy back; this call draws
 *   at the region's own resolution instead (the picture's pixels are never resampled).  VP_ERR_ARG for any kind but VP_EGOLANES, a non-finite
 *   threshold and the geometry / GPU / tensor-input refusals of vp_canvas_blend_mask; VP_ERR_STATE before the engine's first pass.
 * vp_canvas_draw_points: host int xy[n][2] (x, y) in canvas pixels, bgr u8 [3].  Each point sets the disc dx * dx + dy * dy <= radius * radius around it
 *   to the colour, clipped to the canvas; for radius 3 the row half-widths are 3, 2, 2, 0 (dy = 0, 1, 2, 3: 29 pixels).  This rule IS the definition;
 *   like the other OpenCV restatements it is not pinned against cv::circle.  radius 0 .. 16, n 0 .. 4096; n = 0 draws nothing, a point whose disc
 *   lies outside the canvas draws nothing.  VP_ERR_ARG: n < 0 or > 4096, null xy with n > 0, a null colour, a radius out of range.
 * vp_canvas_draw_lane_rows: make_visualization (Models/visualizations/AutoSteer/video_visualization.py:19-44) on a VP_AUTOSTEER engine.  The kernel
 *   reads xp[64] and h_vector[64] from the engine's device logits itself: no D2H, no host wait.  Row i is drawn when h_vector[i] >= 0.5f, as the disc
 *   of vp_canvas_draw_points with radius 3 and BGR (0, 255, 0) around x = x0 + (int)(xp[i] * 1024.0f) (fp32 product, truncation toward zero),
 *   y = y0 + i * 511 / 63 (integer division: numpy.linspace(0, 511, 64, dtype=int)), (x0, y0) the origin of the region the engine's input came from;
 *   the discs are clipped to the canvas.  A row whose product is NaN or not inside (-1e8, 1e8) draws nothing.  Refusals as vp_canvas_blend_mask with
 *   the kinds reversed: VP_ERR_ARG for any kind but VP_AUTOSTEER.  The other two lanes the script keeps commented out, text and curves are not built.
 * vp_canvas_fetch_resized: vp_canvas_fetch of the picture resized to out_h x out_w (each 1 .. 16384) -- the display thread's
 *   cv::resize(unified_frame, display_frame, Size(1280, 720)) -- without a full-size D2H.  The resize is the integer bilinear of VP_RESIZE_CV_LINEAR:
 *   the u8 value the preprocess path forms ahead of normalisation (same tap tables, same device arithmetic; restated by oracle/pre_post.py
 *   resize_bilinear_u8).  The result is a second device picture; format conversion, colour standard, chroma rule and refusals are vp_canvas_fetch's,
 *   applied to (out_h, out_w); vp_canvas_layout3(format, out_h, out_w, ..) answers the planes (for a side of 1, which only the one-plane formats
 *   without chroma pairs take, a plane is out_h rows of pixel bytes x out_w).  The canvas itself is unchanged: later draws and fetches see the
 *   full-size picture.  With (out_h, out_w) the canvas's own geometry the bytes equal vp_canvas_fetch's (the identity taps weigh (2048, 0)).  Host waits
 *   beyond the fetch itself: the once-per-geometry ones of the ORDERING CONTRACT (the second picture growing, the first use of a tap table).
 * vp_canvas_device / vp_canvas_sync: the device picture (BGR8, rows *pitch_bytes apart) for a device consumer such as an encoder; complete after
 *   vp_canvas_sync, valid until the next vp_canvas_begin or vp_canvas_destroy.
 * THE PICTURE AS A BASELINE JPEG, encoded on the device (vp_canvas_fetch_jpeg*, vp_op_jpeg_encode_bgr8): what a visualisation script's
 *   cv2.VideoWriter(.., fourcc "MJPG").write(frame) makes on a host thread, so that a fetch moves the compressed stream instead of the picture.  The
 *   rules below ARE the definition: for a given (picture, quality, Ri) the bytes are a pure function of the input, the same on every call, and
 *   tests/jpeg_ref.py restates them in numpy.  Baseline sequential DCT (ITU-T T.81, SOF0), 8 bits, three components, 4:2:0, JFIF 1.01.
 *   SAMPLES.  The Y, Cb, Cr planes are exactly the bytes vp_canvas_fetch(VP_FRAME_I420) gives under (VP_COLOR_BT601, VP_COLOR_RANGE_FULL, VP_CHROMA_MEAN)
 *   -- JFIF's YCbCr -- whatever vp_canvas_set_color says (the same device functions form them).  w and h are even, 2 .. 16384: the I420 fetch's
 *   refusals, with its texts.  The MCU is 16 x 16 pixels, the grid ceil(w / 16) x ceil(h / 16) MCUs in raster order; samples beyond the picture repeat
 *   the last column / row of their plane (Y and chroma each on their own); an MCU holds six 8 x 8 blocks in the order Y00 Y01 Y10 Y11 Cb Cr;
 *   x = sample - 128.
 *   FORWARD DCT, integer.  M[k][n] = rne(2^13 s_k cos((2n + 1) k pi / 16)) with s_0 = 1 / (2 sqrt 2), s_k = 1 / 2 otherwise, formed in double (2896 for
 *   k = 0, M[1][0] = 4017, |M| <= 4017).  Rows: T[y][k] = (sum_n M[k][n] x[y][n] + 2^9) >> 10; columns: F[l][k] = (sum_m M[l][m] T[m][k] + 2^15) >> 16;
 *   arithmetic shifts, int32 sums (|T| <= 2896, column sums below 2^26; |F - the exact orthonormal DCT| <= 0.65 on the random and extreme blocks of
 *   tests/test_jpeg_host.py, whose bound is 1).
 *   QUANTISATION.  T.81 Annex K.1 (luminance) and K.2 (chrominance), scaled by quality q in 1 .. 100 as libjpeg does: s = q < 50 ? 5000 / q : 200 - 2 q
 *   (integer division), Q = clamp((base * s + 50) / 100, 1, 255); c = sign(F) * ((|F| + (Q >> 1)) / Q).  AC values are clamped to +-1023 (never reached:
 *   tests/test_jpeg_host.py shows it from M's row sums).  Coefficients are taken in zigzag order.
 *   ENTROPY CODING (T.81 F.1.2) with the four typical Huffman tables of Annex K.3.3 (K.3 .. K.6): luminance DC 0 / AC 0, both chroma components DC 1 /
 *   AC 1.  DC: the difference to the previous block of the same component, predictor 0 at the start of every restart interval; the category's code, then
 *   SSSS low bits (a negative value sends v - 1).  AC: (run, size) symbols, ZRL = 0xF0, EOB = 0x00 only when the block ends in zeros.  Bits MSB first, a
 *   0x00 stuffed behind every 0xFF data byte, each interval padded to a byte boundary with 1-bits.
 *   RESTART INTERVALS.  restart_mcus (Ri) 1 .. 65535 MCUs in raster order; between interval i and i + 1 the marker RST(i mod 8), none behind the last.
 *   restart_mcus = 0 selects the default, 4 (profiles/canvas_jpeg.txt: the fastest of 1, 2, 4, 8 whose size stays within 5 % of Ri = 8).  An interval is
 *   what one work-item of the entropy kernel codes, so Ri trades parallelism against marker bytes.
 *   LAYOUT.  SOI; APP0 "JFIF\0" (1.01, units 0, density 1:1, no thumbnail); DQT table 0, DQT table 1 (8-bit, zigzag); SOF0 (precision 8, h, w,
 *   {1: 2x2 Tq 0, 2: 1x1 Tq 1, 3: 1x1 Tq 1}); four DHT (DC 0, AC 0, DC 1, AC 1); DRI (always); SOS (Ss 0, Se 63, Ah / Al 0); scan data; EOI.  The
 *   header, SOI through SOS, has 629 bytes whatever the arguments.
 *   vp_canvas_fetch_jpeg: synchronous; the stream into dst [cap], its length in *n.  The canvas is unchanged: later draws and fetches see the same
 *   picture.  The header is written on the host straight into dst; the scan is coded on the device behind the canvas's stream order.  Host waits: two,
 *   one for the scan's length and one for its bytes (beyond them the once-per-geometry ones of the ORDERING CONTRACT: the encoder's buffers growing).
 *   VP_ERR_ARG with text: null dst / n, quality outside 1 .. 100, restart_mcus outside 0 .. 65535, the geometry refusals above, and a cap below the
 *   stream's length -- decided before any byte of dst beyond the header is written; the text names the length and *n receives it (the one thing a
 *   refused call stores).  vp_jpeg_bound answers a cap that always suffices.  VP_ERR_STATE before the first vp_canvas_begin.
 *   vp_canvas_fetch_jpeg_resized: the JPEG of the second picture vp_canvas_fetch_resized forms (out_h, out_w even, 2 .. 16384): the production display's
 *   1280 x 720.  vp_op_jpeg_encode_bgr8 (declared with the operator entries below) is the same encoder on a host picture, without frame or canvas.
 *   Not built: 4:4:4 / 4:2:2 / grey, per-picture Huffman tables, progressive mode, a decoder; an MJPG / AVI container is a few host bytes per frame.
 * ORDERING CONTRACT (vp_frame's, in the other direction).  Nothing waits on the host before vp_canvas_fetch / vp_canvas_sync.  A draw call makes the
 *   canvas's stream wait for the work queued on the engine's stream so far, and the engine's stream wait for the canvas's read of the mask / logits
 *   before anything queued on it afterwards: `infer A; blend; infer B; fetch` shows A's mask.  The exceptions are once per geometry: a buffer that
 *   has to grow, and the first use of a resize table of a new (network size, region size) pair, which is uploaded and waited for.
 * THREADING.  One thread drives a canvas; a draw call is also a call on the engine it names (one thread at a time per engine, as ever).  No
 *   process-wide state. */
typedef struct vp_canvas vp_canvas;
struct vp_detection;   /* the detector's record, defined with the detector below */
int vp_canvas_create(vp_canvas** out, int gpu_id, char* err, size_t err_len);
void vp_canvas_destroy(vp_canvas* c);
const char* vp_canvas_last_error(const vp_canvas* c);
int vp_canvas_begin(vp_canvas* c, vp_frame* f);
int vp_canvas_blend_mask(vp_canvas* c, vp_engine* e, int viz_type);
int vp_canvas_blend_mask_u8(vp_canvas* c, const uint8_t* mask, int mask_on_device, int mh, int mw, int viz_type, int x0, int y0, int w, int h);
int vp_canvas_paste_depth(vp_canvas* c, vp_engine* e);
int vp_canvas_draw_detections(vp_canvas* c, const struct vp_detection* dets, int n);
int vp_canvas_sync(vp_canvas* c);
int vp_canvas_dims(const vp_canvas* c, int* h, int* w);                  /* VP_ERR_STATE before the first vp_canvas_begin */
int vp_canvas_device(const vp_canvas* c, void** dev_bgr8, int* pitch_bytes);
int vp_canvas_layout(int format, int h, int w, int* n_planes, int row_bytes[2], int rows[2]);   /* host only */
int vp_canvas_layout3(int format, int h, int w, int* n_planes, int row_bytes[3], int rows[3]);  /* host only; every format */
int vp_canvas_set_color(vp_canvas* c, int matrix, int range, int chroma_mode);   /* applies to later fetches; not inherited from the frame */
int vp_canvas_get_color(const vp_canvas* c, int* matrix, int* range, int* chroma_mode);
int vp_canvas_fetch(vp_canvas* c, int format, uint8_t* const* planes, const int* strides, int n_planes);
int vp_canvas_add_planes_f32(vp_canvas* c, const float* planes, int planes_on_device, int n_planes, int mh, int mw, float threshold, const uint8_t* add_bgr, int x0,
                             int y0, int w, int h);
int vp_canvas_overlay_lanes(vp_canvas* c, vp_engine* egolanes, float threshold);
int vp_canvas_draw_points(vp_canvas* c, const int* xy, int n, int radius, const uint8_t* bgr);
int vp_canvas_draw_lane_rows(vp_canvas* c, vp_engine* autosteer);
int vp_canvas_fetch_resized(vp_canvas* c, int format, int out_h, int out_w, uint8_t* const* planes, const int* strides, int n_planes);
int vp_canvas_fetch_jpeg(vp_canvas* c, int quality, int restart_mcus, uint8_t* dst, size_t cap, size_t* n);
int vp_canvas_fetch_jpeg_resized(vp_canvas* c, int out_h, int out_w, int quality, int restart_mcus, uint8_t* dst, size_t cap, size_t* n);
/* host only, no device: an upper bound of the stream's length for (h, w, restart_mcus) -- 629 + 2 + 2490 bytes per MCU (six blocks of at most
 * 22 + 63 * 26 bits, every byte stuffed) + 2 per interval -- and the header, SOI through SOS (629 bytes into dst [cap], *n = 629).  Refusals as above. */
int vp_jpeg_bound(int h, int w, int restart_mcus, size_t* bytes, char* err, size_t err_len);
int vp_jpeg_header(int h, int w, int quality, int restart_mcus, uint8_t* dst, size_t cap, size_t* n, char* err, size_t err_len);

/* ---- vp_metric: the reference's validation scores, computed on the device, one small record per frame -----------------------------
 * The reference qualifies its runtimes by task score: the IoU of SceneSegTrainer.calc_IoU_val / IoU (Models/training/scene_seg_trainer.py:206-244,
 * domain_seg_trainer.py:236-252) and the mAE / mEL of Scene3DTrainer.validate (scene_3d_trainer.py:94-109, 159-162, 171-210, 295-319).  A vp_metric is a
 * per-GPU accumulator of those scores: an add call reads an engine's device-resident logits behind its pass (as a vp_canvas draw does) or a caller's
 * tensors, queues a few kernels on the metric's own stream and returns; a run over a dataset costs ONE fetch at the end.
 *     vp_metric_create(&m, 0, n_frames, err, sizeof err);
 *     for each frame:  vp_infer(seg, ...);  vp_metric_add_seg(m, seg, gt, 0, VP_GT_LABEL);      no host wait
 *     vp_metric_fetch(m, records, n_frames, &summary);                                            the one synchronisation
 * SEGMENTATION.  Prediction, C = 3: class 0 if l0 >= l1 && l0 >= l2, else 1 if l1 >= l0 && l1 >= l2, else 2 if l2 >= l0 && l2 >= l1 (the first maximum
 *   for finite logits); C = 1: positive (class 0 of the record) where logit > 0.  Ground truth, u8 of the output's size: VP_GT_LABEL -- the value is the
 *   class index, a value >= C is no class (C = 1: nonzero is positive); VP_GT_BITS -- bit c is plane c, planes may overlap (the reference's stacked
 *   one-hot planes).  Counts per class c, u32: I[c] = #(pred == c and gt_c), P[c] = #(pred == c), G[c] = #gt_c; U[c] = P[c] + G[c] - I[c].  Scores, double
 *   on the host: iou[c] = (I[c] + 1) / (U[c] + 1), iou_full = (sum I + 1) / (sum U + 1) (C = 1: both coincide); the dataset score is the mean over the
 *   frames of the per-frame scores (train_scene_seg.py, benchmark_onnx_models.py).
 *   DEPARTURE 1: a pixel with a NaN logit fails all three branches; it predicts NO class and is counted in `nonfinite` (C = 1: a NaN logit is not
 *   positive and is counted).  The reference leaves the raw values in its one-hot planes there.
 * DEPTH.  Plane 0 of the logits (p) and an fp32 plane g of the same size; ssi(t) = (t - min t) / (max t - mean t) on both; D = ssi(p) - ssi(g), A = |D|.
 *   mAE: q = the 0.9 quantile of A, linear interpolation between the order statistics q_lo = A_(lo) and q_hi = A_(min(lo + 1, n - 1)), lo = floor(r),
 *   r = fp32(0.9f * (n - 1)), weight w = r - lo, evaluated as torch.lerp does in fp32 (q_lo + w (q_hi - q_lo) for w < 0.5, q_hi - (q_hi - q_lo)(1 - w)
 *   otherwise); mae = mean of the elements of A STRICTLY below q (`kept` of them: elements equal to q are excluded, so with q_lo == q_hi the kept set is
 *   {A < q_lo}).  mEL: the mean over four scales of mean(|Gx(D)| + |Gy(D)|) -- scale 0 the plane, scales 1 .. 3 2x2 mean pools with stride 2 (a trailing
 *   odd row or column dropped), Gx / Gy the 3x3 filters of lines 96-106 with zero padding 1; the filters and pools are applied to D, the same linear map
 *   as the reference's difference of filtered planes.  What the reference answers, this answers: p identical to g gives a NaN mae (an empty mean) and
 *   mel 0; a constant plane gives NaN for both.  A non-finite input value gives NaN scores and a `nonfinite` count.
 *   DEPARTURE 2: the dataset score (the mean of the per-frame mae and mel, train_scene_3d.py:161-172) leaves frames with a NaN mae or mel out of both
 *   means and reports them in nan_frames; the reference would propagate the NaN.
 * vp_metric_create: max_frames records (1 .. 1 << 20) on gpu_id; VP_ERR_ARG / VP_ERR_HIP with the text in err.
 * vp_metric_add_seg / vp_metric_add_depth: VP_SCENESEG and VP_DOMAINSEG / VP_SCENE3D engines, shared-prefix heads included; gt has the engine's output
 *   size (vp_output_dims) and lies in host memory (copied before the call returns) or, gt_on_device != 0, in complete device memory on the metric's GPU.
 * vp_metric_add_seg_pair / vp_metric_add_depth_pair: ref's own prediction (its class by the rule above / its plane 0) is the ground truth.
 * vp_metric_add_seg_logits / vp_metric_add_depth_plane: the operator entries -- the same kernels on a caller's fp32 tensors (logits [c][h][w], c 1 or 3;
 *   planes [h][w]) of any size with h * w <= 1 << 24; the record's kind is VP_SCENESEG (c = 3), VP_DOMAINSEG (c = 1) or VP_SCENE3D.
 * vp_metric_fetch: waits for the metric's stream, copies the first min(cap, frames) records (records may be NULL with cap 0) and fills *summary (may be
 *   NULL) from ALL records.  vp_metric_reset empties the accumulator (queued work stays ordered); vp_metric_frames: records added since.
 * Records are bit-identical from run to run: integer counters, partial sums folded in a fixed order.
 * ERRORS.  VP_ERR_ARG: another engine kind, an engine on another GPU, a pair of different kinds or sizes, h or w below 8 in the depth entries, h * w above
 *   1 << 24, c outside {1, 3}, an unknown gt_form, a null pointer.  VP_ERR_STATE: an engine with no pass yet, a full accumulator.
 * ORDERING CONTRACT: the canvas's.  An add call makes the metric's stream wait for the work queued on the engine's stream so far, and the engine's stream
 *   wait for the metric's read before anything queued on it afterwards (both engines in the pair forms).  No add call waits for the device, with the
 *   once-per-geometry exceptions of a scratch or staging buffer that has to grow, and a pinned staging slot still read by the copy of two calls earlier.
 * THREADING.  One thread drives a metric; an add call is also a call on the engines it names.
 * vp_op_select_f32: the chain's radix select alone -- *out = the k-th smallest (k = 0 .. n - 1) of n (1 .. 1 << 24) non-negative finite host floats,
 *   bit for bit; VP_ERR_ARG for a negative (-0.0f included) or non-finite value. */
typedef struct vp_metric vp_metric;
enum vp_gt_form { VP_GT_LABEL = 0, VP_GT_BITS = 1 };
typedef struct vp_metric_frame {
  int kind;                       /* VP_SCENESEG, VP_DOMAINSEG or VP_SCENE3D */
  uint32_t I[3], P[3], G[3];      /* segmentation counts (C = 1: index 0) */
  uint32_t nonfinite;             /* pixels with a NaN logit / non-finite values of the two depth planes */
  uint32_t n;                     /* h * w */
  uint32_t kept;                  /* depth: elements of A below q */
  float q_lo, q_hi, q, mae, mel;  /* depth */
} vp_metric_frame;
typedef struct vp_metric_summary {
  int frames, sceneseg_frames, domainseg_frames, scene3d_frames;
  int nan_frames;                 /* VP_SCENE3D records left out of mae / mel */
  int reserved;
  double sceneseg_iou[3], sceneseg_iou_full, domainseg_iou, mae, mel;   /* means over the frames of the kind; NaN where there is none */
} vp_metric_summary;
int vp_metric_create(vp_metric** out, int gpu_id, int max_frames, char* err, size_t err_len);
void vp_metric_destroy(vp_metric* m);
const char* vp_metric_last_error(const vp_metric* m);
int vp_metric_reset(vp_metric* m);
int vp_metric_add_seg(vp_metric* m, vp_engine* e, const uint8_t* gt, int gt_on_device, int gt_form);
int vp_metric_add_depth(vp_metric* m, vp_engine* e, const float* gt, int gt_on_device);
int vp_metric_add_seg_pair(vp_metric* m, vp_engine* e, vp_engine* ref);
int vp_metric_add_depth_pair(vp_metric* m, vp_engine* e, vp_engine* ref);
int vp_metric_frames(const vp_metric* m);
int vp_metric_fetch(vp_metric* m, vp_metric_frame* records, int cap, vp_metric_summary* summary);
int vp_metric_add_seg_logits(vp_metric* m, const float* logits_chw, int on_device, int c, int h, int w, const uint8_t* gt, int gt_on_device, int gt_form);
int vp_metric_add_depth_plane(vp_metric* m, const float* pred, int pred_on_device, const float* gt, int gt_on_device, int h, int w);
int vp_op_select_f32(int gpu_id, const float* values, int n, int k, float* out, char* err, size_t err_len);

/* ---- vp_metric: the detector's validation mAP --------------------------------------------------------------------------------------
 * The detector's trainer validates with non_max_suppression at conf 0.001 / iou 0.65, compute_metric and compute_ap (Models/training/
 * auto_speed_trainer.py:176-229, auto_speed_util.py:99-169, 225-300): precision, recall, mAP@50 and mAP.  That post-process is NOT the inference one
 * (vp_detect_postprocess*): it is multi-label, offsets boxes per class, ranks up to 43 008 candidates and keeps at most 300.  The same vp_metric handle
 * accumulates it: one small record, the kept rows and the label classes per frame on the device, ONE vp_metric_fetch_det per dataset run.  Detector
 * records are counted apart (vp_metric_det_frames); vp_metric_fetch / _frames / vp_metric_frame / vp_metric_summary know nothing of them.
 * THE PER-FRAME STAGE.  Input: raw[4 + nc][nb] fp32, rows cx, cy, w, h, score_0 .. score_{nc-1}; nc 1 .. 80, nb 1 .. 16384, nb * nc <= 131072.  Every
 *   floating operation below is a single IEEE fp32 operation in the order written, without contraction.
 *   Candidates: every pair (box i, class c) with score > conf; a NaN score is no candidate.  Candidate order is i major, c minor (nc == 1: the
 *     reference's "best class" branch gives the same set).
 *   Rank: by descending score.  TIE DEFINITION 1: equal scores keep candidate order (the reference's argsort leaves it open).  The first
 *     VP_DET_MAX_NMS candidates go on (`ranked`); `candidates` reports how many there were.
 *   Corners: x1 = cx - w / 2, y1 = cy - h / 2, x2 = cx + w / 2, y2 = cy + h / 2.  The suppression box is each corner + (float)c * 7680.0f.
 *   Suppression: greedy in rank order with torchvision's rule on the offset boxes: iw = max(0, min(x2) - max(x1)), ih likewise (fmaxf / fminf),
 *     inter = iw * ih; a later box j is suppressed by a kept box i when inter / (area_i + area_j - inter) > iou.  0 / 0 is NaN and suppresses
 *     nothing.  It stops when VP_DET_MAX_DET boxes are kept or the list ends.
 *   Output: per kept row the un-offset corners, the score and the class.
 *   Labels: n_labels (0 .. 4096) rows [cls, cx, cy, w, h] in the reference's dataset form, normalised to the network input W x H; the device forms the
 *     corners as above and multiplies by (W, H, W, H).
 *   Matching (compute_metric): for label l and detection d, iw = min(x2_l, x2_d) - max(x1_l, x1_d) and ih likewise, each replaced by 0 when negative
 *     (a NaN stays), inter = iw * ih, iou = inter / (((area_l + area_d) - inter) + 1e-7f), areas = (x2 - x1) * (y2 - y1).  For threshold t of the
 *     caller's table iou_v[n_iou] (n_iou 1 .. 16) a pair is eligible when iou >= t and cls_l == cls_d as floats.  Each detection's best label is its
 *     eligible pair of highest IoU (TIE DEFINITION 2: of equal IoUs the label of lowest index; the reference leaves it to an unstable argsort).  Among
 *     the detections whose best label is l, the one of LOWEST INDEX (highest score) is correct at t -- not the one of highest IoU: this is what the two
 *     numpy.unique(..., return_index=True) calls of compute_metric leave, and it is NOT the usual greedy rule.  Bit t of the row's `tp` word says so.
 *   Threshold table: the library takes it from the caller and does not recompute it.  The trainer's is torch.linspace(0.5, 0.95, 10), whose bits are
 *     3f000000 3f0ccccd 3f19999a 3f266666 3f333333 3f400000 3f4ccccd 3f59999a 3f666666 3f733333.  One table per dataset run: an add with another table
 *     than the records so far is refused.
 *   Frame bookkeeping (auto_speed_trainer.py:208-219): a frame with no kept row and no label adds nothing to the dataset; no kept row but labels: only
 *     its label classes; kept rows and no labels: its rows with tp = 0.  Every frame still gets its vp_metric_det_frame.
 * DEPARTURE: the trainer's validate() runs the model and the NMS in half precision.  This stage scores the engine's fp32 tensor with fp32 arithmetic,
 *   which is what non_max_suppression does on a float tensor.
 * vp_metric_add_det: e is a VP_AUTOSPEED engine with a pass behind it; its raw tensor (vp_logits) is read on the device under the ordering contract of
 *   vp_metric_add_seg.  labels are host floats, copied before the call returns; n_labels may be 0 (labels may then be NULL).  W x H is the engine's input.
 * vp_metric_add_det_pair: the labels are ref's own kept rows (the same stage on ref's tensor at conf / iou) with score > label_conf, formed on the
 *   device; they are in pixels already.
 * vp_metric_add_det_raw: the operator entry on a caller's tensor, in host memory (copied before return) or, on_device != 0, device memory on the
 *   metric's GPU.
 * vp_metric_det_frames: detector frames added since the last reset.  Capacity: min(max_frames, 16384) frames and 64 labels per frame of capacity
 *   (+ 4096) in all; the pair form counts 300 labels per frame against it.  vp_metric_reset empties the detector storage too.
 * vp_metric_fetch_det: the one synchronisation.  Copies the first min(frames_cap, frames) frame records and the first min(rows_cap, rows) kept rows
 *   (frame f's rows are rows[first_row .. first_row + kept), in rank order) and fills *summary (may be NULL) from ALL of them.
 * vp_metric_det_summary is computed on the host in double exactly as compute_ap does: rows sorted by -conf; the classes are those of the LABELS only,
 *   ascending; cumulative sums; recall = tpc / (n_labels + 1e-16), precision = tpc / (tpc + fpc), both interpolated (numpy.interp) at
 *   numpy.linspace(0, 1, 1000) over -conf with left = 0 / left = 1; per threshold the precision envelope, the 101-point interp and trapz; f1 =
 *   2 p r / (p + r + 1e-16); grid_index = the first maximum of smooth(f1.mean(0), 0.1) (a 101-tap box filter over the edge-padded curve); precision and
 *   recall are the class means at that index, tp = round(r * n_labels), fp = round(tp / (p + 1e-16) - tp) (half to even), map50 / map the class means
 *   of ap50 / ap.  If no row has a tp bit set the four scores are 0 and grid_index is -1, as the trainer's `metrics[0].any()` decides.  The per-class
 *   arrays hold the first VP_DET_MAX_CLASSES label classes; `classes` counts all and the means run over all.  The plots of compute_ap are not made.
 * vp_metric_det_ap: the same host code over caller arrays (tp words, conf, detection classes [n_rows]; label classes [n_labels]); no device, no handle.
 * vp_op_detect_validate: the candidate / rank / suppression part alone on a host tensor: rows [x1, y1, x2, y2, score, cls] (the first min(cap, kept)
 *   of them) and counts_out = {candidates, ranked, kept}.
 * Records are bit-identical from run to run: the one atomic slot counter only places keys that the rank (which depends on the SET of keys) reorders.
 * ERRORS.  VP_ERR_ARG: another engine kind, an engine on another GPU, sizes beyond the limits above, n_iou outside 1 .. 16, another table than before, a
 *   NaN threshold, a null pointer, a pair of different nc / nb.  VP_ERR_STATE: an engine with no pass yet, a full accumulator. */
#define VP_DET_MAX_NMS 30000
#define VP_DET_MAX_DET 300
#define VP_DET_MAX_CLASSES 80
#define VP_DET_MAX_IOU 16
#define VP_DET_MAX_LABELS 4096
typedef struct vp_metric_det_frame {
  uint32_t candidates, ranked, kept, labels, first_row;
} vp_metric_det_frame;
typedef struct vp_metric_det_row {
  float x1, y1, x2, y2, conf, cls;
  uint32_t tp;                    /* bit t: correct at iou_v[t] */
} vp_metric_det_row;
typedef struct vp_metric_det_summary {
  int frames, rows, labels;
  int classes;                    /* distinct label classes */
  int n_iou;
  int grid_index;                 /* on the 1000-point confidence grid; -1: not scored */
  double precision, recall, map50, map;
  float class_id[VP_DET_MAX_CLASSES];
  uint32_t class_labels[VP_DET_MAX_CLASSES];
  double ap50[VP_DET_MAX_CLASSES], ap[VP_DET_MAX_CLASSES], tp[VP_DET_MAX_CLASSES], fp[VP_DET_MAX_CLASSES];
} vp_metric_det_summary;
int vp_metric_add_det(vp_metric* m, vp_engine* e, const float* labels, int n_labels, float conf, float iou, const float* iou_v, int n_iou);
int vp_metric_add_det_pair(vp_metric* m, vp_engine* e, vp_engine* ref, float label_conf, float conf, float iou, const float* iou_v, int n_iou);
int vp_metric_add_det_raw(vp_metric* m, const float* raw, int on_device, int nc, int nb, int net_h, int net_w, const float* labels, int n_labels, float conf, float iou,
                          const float* iou_v, int n_iou);
int vp_metric_det_frames(const vp_metric* m);
int vp_metric_fetch_det(vp_metric* m, vp_metric_det_frame* frames_out, int frames_cap, vp_metric_det_row* rows_out, int rows_cap, vp_metric_det_summary* summary);
int vp_metric_det_ap(const uint32_t* tp, const float* conf, const float* det_cls, int n_rows, const float* label_cls, int n_labels, int n_iou, vp_metric_det_summary* summary);
int vp_op_detect_validate(int gpu_id, const float* raw, int nc, int nb, float conf, float iou, float* rows_out, int cap, uint32_t* counts_out, char* err, size_t err_len);

/* ---- vp_metric: the lane networks' validation scores -----------------------------------------------------------------------------------
 * EgoLanes validates with the mean of its training loss over the samples (Models/training/ego_lanes_trainer.py:127-140, 214-222, 280-356;
 * train_ego_lanes.py:387-417); AutoSteer with a per-line distance, three thresholds and compute_vector_ap (auto_steer_trainer.py:176-248,
 * auto_steer_util.py:353-399).  The same vp_metric handle accumulates both, each in records of its own, counted apart (vp_metric_lanes_frames,
 * vp_metric_rows_lines): vp_metric_fetch / _frames / vp_metric_frame / vp_metric_summary and the detector entries know nothing of them, and
 * vp_metric_add_seg keeps refusing a VP_EGOLANES engine.  VP_AUTODRIVE has no entry: its output is three scalars the host already holds.
 * LANE MASKS (EgoLanes).  Logits x fp32 [3][h][w] and a ground truth g of three planes.  Per plane c, every floating operation in fp32 unless said:
 *   bce_c  = mean of (1 - g) x + max(-x, 0) + log1p(exp(-|x|))    (BCEWithLogitsLoss; exp and log1p are the device library's, so this term is not
 *            defined bit for bit; the per-pixel terms are summed in double)
 *   R = x where x > 0, else 0 (relu);  T = R where R > 0, else 1.0 (torch.nn.Threshold(0, 1): NOT a step function -- a negative or zero logit gives 1.0)
 *   e_0    = mean(|Gx(R - g)| + |Gy(R - g)|);   e_s, s = 1 .. 4: the same of P^s(T - g), P the 2x2 mean pool of stride 2 (0.25 ((a + b) + (c + d)); a
 *            trailing odd row or column dropped), Gx / Gy the 3x3 filters of lines 127-140 with zero padding 1 in the expression of the depth
 *            entries.  The filters and pools are applied to the difference, the same linear map as the trainer's difference of filtered planes.
 *   edge_c = ((((e_0 + e_1) + e_2) + e_3) + e_4) / 5;   loss_c = edge_c + bce_c;   score = (2 loss_0 + 2 loss_1) + loss_2.
 *   Every mean is one fp32 division of the sum (formed in double, partials folded in a fixed order, rounded to fp32) by the count.
 *   Ground truth forms (gt_form), each in host memory (copied before the call returns) or, gt_on_device != 0, complete device memory on the metric's GPU:
 *     VP_LANES_GT_PLANES   fp32 [3][h][w], any finite values;
 *     VP_LANES_GT_BITS     u8 [h][w], bit c is plane c (VP_GT_BITS of the output size);
 *     VP_LANES_GT_BITS_4X  u8 [4h][4w] (the dataset's 320 x 640 label for the 80 x 160 output): plane c of a pixel is bit c of the OR over its 4x4
 *                          block -- the two MaxPool2d(2, 2) of lines 220-222 on binary planes.
 *   DEPARTURE 3: a non-finite logit or fp32 ground-truth value makes every score of the frame NaN and is counted in `nonfinite`; the dataset means leave
 *   such frames out and report them in nan_frames.  The trainer would propagate the NaN (or, for an infinite logit, answer inf).
 *   DEPARTURE 4: the trainer's validation runs the model as its training does; this scores the engine's fp32 logits, whatever precision produced them.
 *   vp_metric_add_lanes: e is a VP_EGOLANES engine with a pass behind it; its logits are read on the device under the ordering contract of
 *     vp_metric_add_seg (the canvas's, unchanged).  The ground truth has the output's size (vp_output_dims), or four times it.
 *   vp_metric_add_lanes_pair: the ground truth is ref's own prediction: planes of 1 where ref's logit > 0, else 0 (a NaN gives 0 and is not counted).
 *   vp_metric_add_lanes_logits: the operator entry on a caller's logits [3][h][w], host or device; h, w >= 16 (scale 4 has a pixel) and h * w <= 1 << 22.
 *     Planes of at most 12 800 pixels (the production 80 x 160) take two launches, larger ones seven; the scores are defined alike.
 *   vp_metric_fetch_lanes: the one synchronisation.  Copies the first min(cap, frames) records and fills *summary (may be NULL) from ALL of them, in
 *     double on the host: the means over the frames without NaN of score, loss_c, bce_c and edge_c = (e_0 + .. + e_4) / 5 (NaN where there is none).
 * LANE ROWS (AutoSteer).  Per line, rows values each of xp, h_vector, target_xp, target_h (the 'n' network: one line of 64 rows per frame, logits
 *   {1, 2, 64, 1} = xp, then h_vector):
 *   m = h_vector > 0.5, mt = target_h > 0.5 (a NaN is not valid);  term_r = |xp_r * m_r - target_xp_r * mt_r| as fp32 operations;
 *   dist = fp32(sum(term) / rows), conf = fp32(sum(h_vector) / rows).  SUMMATION ORDER: the sums are formed in double; element r is added to slot
 *   r mod 256 in ascending r, then the 256 slots fold as slot i += slot i + o for o = 128, 64, .. 1; the quotient is a double division, rounded once.
 *   Bit t of `tp` is (double)dist < thr[t]: the comparison in double against the fp32 value, as the trainer's .item() makes it.  `valid` and
 *   `target_valid` count m and mt.  A NaN in xp or a target gives a NaN dist and no tp bit, as the trainer would.
 *   Threshold table: the caller's, 1 .. 8 doubles, none NaN (the trainer's is {0.02, 0.05, 0.10}).  One table per run: an add with another table than the
 *   lines so far is refused until vp_metric_reset.
 *   DEPARTURE 5: the trainer's val() runs the model in half precision; this scores the engine's fp32 tensor with the arithmetic above.
 *   vp_metric_add_rows: e is a VP_AUTOSTEER engine with a pass behind it; target_xp / target_h are host floats [rows], copied before the call returns.
 *   vp_metric_add_rows_pair: the targets are ref's own rows (its xp and h_vector), read on the device.
 *   vp_metric_add_rows_raw: the operator entry on host arrays [n_lines][rows], n_lines 1 .. 8, rows 1 .. 1024; one record per line, in order.
 *   vp_metric_fetch_rows: the one synchronisation; the first min(cap, lines) records and *summary (may be NULL) from ALL lines with the run's table.
 *   vp_metric_rows_ap: the summary's host code over caller arrays (tp words, conf [n_lines]); no device, no handle.  It is compute_vector_ap in
 *     double: per table entry t the lines sorted by descending conf (TIE DEFINITION: equal conf keep line order -- the reference's argsort leaves it
 *     open; a NaN conf goes last), tpc / fpc the running counts of set / clear tp bits, precision = tpc / (tpc + fpc + 1e-16), recall =
 *     tpc / (lines + 1e-16), the precision envelope over {0, recall, 1} / {0, precision, 0}, numpy.interp at numpy.linspace(0, 1, 101) and the
 *     trapezoid sum: ap[t].  precision / recall: the mean over the entries of the means over the lines; mean_ap: the mean of ap[t]; map50: the ap of the
 *     entry equal to 0.05 as a double, NaN if the table has none.  Entries are taken in table order (the reference sorts its three ascending).
 *     No lines: the four scores are 0, as val() answers.
 * Capacity: max_frames lane-mask frames and max_frames lines.  vp_metric_reset empties both.  Records are bit-identical from run to run: no atomics, one
 *   partial per workgroup, folded by the next launch in index order (bce_c up to the device library's exp / log1p, which are deterministic as well).
 * ERRORS.  VP_ERR_ARG: another engine kind, an engine on another GPU, a pair of different sizes, h or w below 16, h * w above 1 << 22, an unknown gt_form,
 *   a device pointer not aligned to 4 bytes (logits, fp32 planes, the 4x form), n_lines / rows / n_thr outside their ranges, a NaN threshold, another
 *   table than the run's, a null pointer.  VP_ERR_STATE: an engine with no pass yet, a full accumulator.
 * No add call waits for the device beyond the exceptions of vp_metric_add_seg (a scratch or staging buffer that has to grow, a pinned slot in use) and
 *   the allocation of the record storage by the first add of either kind. */
enum vp_lanes_gt_form { VP_LANES_GT_PLANES = 0, VP_LANES_GT_BITS = 1, VP_LANES_GT_BITS_4X = 2 };
#define VP_ROWS_MAX_THR 8
#define VP_ROWS_MAX_LINES 8
#define VP_ROWS_MAX_ROWS 1024
typedef struct vp_metric_lanes_frame {
  float bce[3], edge[3][5], loss[3], score;
  uint32_t n;                     /* h * w */
  uint32_t nonfinite;             /* non-finite logits and fp32 ground-truth values */
} vp_metric_lanes_frame;
typedef struct vp_metric_lanes_summary {
  int frames;
  int nan_frames;                 /* left out of the means */
  double score, loss[3], bce[3], edge[3];
} vp_metric_lanes_summary;
typedef struct vp_metric_rows_line {
  float dist, conf;
  uint32_t tp;                    /* bit t: dist < thr[t] */
  uint32_t valid, target_valid;   /* rows with h_vector > 0.5 / target_h > 0.5 */
} vp_metric_rows_line;
typedef struct vp_metric_rows_summary {
  int lines, n_thr;
  double precision, recall, mean_ap, ap[VP_ROWS_MAX_THR], map50;
} vp_metric_rows_summary;
int vp_metric_add_lanes(vp_metric* m, vp_engine* e, const void* gt, int gt_on_device, int gt_form);
int vp_metric_add_lanes_pair(vp_metric* m, vp_engine* e, vp_engine* ref);
int vp_metric_add_lanes_logits(vp_metric* m, const float* logits_chw, int on_device, int h, int w, const void* gt, int gt_on_device, int gt_form);
int vp_metric_lanes_frames(const vp_metric* m);
int vp_metric_fetch_lanes(vp_metric* m, vp_metric_lanes_frame* records, int cap, vp_metric_lanes_summary* summary);
int vp_metric_add_rows(vp_metric* m, vp_engine* e, const float* target_xp, const float* target_h, const double* thr, int n_thr);
int vp_metric_add_rows_pair(vp_metric* m, vp_engine* e, vp_engine* ref, const double* thr, int n_thr);
int vp_metric_add_rows_raw(vp_metric* m, const float* xp, const float* h_vector, const float* target_xp, const float* target_h, int n_lines, int rows, const double* thr,
                           int n_thr);
int vp_metric_rows_lines(const vp_metric* m);
int vp_metric_fetch_rows(vp_metric* m, vp_metric_rows_line* records, int cap, vp_metric_rows_summary* summary);
int vp_metric_rows_ap(const uint32_t* tp, const float* conf, int n_lines, const double* thr, int n_thr, vp_metric_rows_summary* summary);

/* ---- vp_metric: ground truth from the datasets' label files, built on the device ------------------------------------------------------
 * The entries above take ground truth that already has the network's output geometry.  The reference makes it on the host, per sample: extractROI
 * crops the label with a PIL box, createGroundTruth walks the crop pixel by pixel in Python against nine colours and counts the class frequencies
 * (Models/data_utils/load_data_scene_seg.py:55-166), A.Resize(640, 320) shrinks each plane with the nearest rule (augmentations.py:133-177); the depth
 * loader min-max normalises a full-resolution .npy map, which is then resized (load_data_scene_3d.py:59-66); DomainSeg's label is an L image through
 * the same resize (load_data_domain_seg.py:57-61).  These entries take the label file's decoded pixels as the dataset stores them and queue all of
 * that on the metric's stream in front of the score: one vp_metric_frame per call as ever (vp_metric_fetch), and one vp_label_frame per call, in call
 * order, in storage of its own (vp_metric_fetch_labels; vp_metric_fetch / vp_metric_frame / vp_metric_summary know nothing of it).
 *     vp_infer(seg, ...);  vp_metric_add_seg_label(m, seg, rgb, 3, h, w, 3 * w, box, &table[0][0], 9);      no host wait
 * ARITHMETIC.
 *   Crop box {l, t, r, b} in PIL's sense: cw = r - l, ch = b - t, crop pixel (y, x) is image pixel (t + y, l + x); NULL: the whole image.  The box may
 *     exceed the image: crop pixels outside it read as (0, 0, 0) / 0, as PIL.Image.crop pads (the reference's (0, 0, 1919, 990) drops the last column;
 *     (0, 476, 2047, 1500) on a shorter image pads, and black, the "unlabelled" colour, is background).
 *   Sampling: output pixel (oy, ox) of the oh x ow ground truth takes crop pixel (ty[oy], tx[ox]), t[d] = min(floor(d * (1 / (dst / src))), src - 1) in
 *     double: OpenCV's resizeNN as vp_mask_resized reads it, from ch -> oh and cw -> ow.  oh x ow is the engine's output size (vp_output_dims).
 *   Colour labels (channels 3; bytes R, G, B as the file has them): the table is n_colours (1 .. 16) rows {r, g, b, class}, class 0 .. 2; a pixel's
 *     class is that of the FIRST row it equals exactly, no row: no class.  The ground truth byte is the class, or 255 (VP_GT_LABEL, as vp_metric_add_seg
 *     reads it).  Classifying after sampling equals the reference's sampling of classified planes: both maps are per pixel.  VP_SCENESEG_COLOURS_INIT is the
 *     reference's table: class 0 sky, background objects, road-edge delimiter, unlabelled; class 1 the four foreground colours; class 2 road.
 *     Statistics over the FULL-RESOLUTION crop: freq[c] pixels of class c, unmatched (inside the image, no row), outside (crop pixels outside the image;
 *     they are ALSO counted in the class of black, if it has one), n = cw * ch.  The reference's loss weights n / (freq[c] + 5120) are host arithmetic.
 *   Mask labels (channels 1): the ground truth byte is the sampled byte (VP_GT_LABEL with one plane: nonzero is positive); freq[0] is the number of
 *     nonzero pixels of the crop, freq[1] = freq[2] = unmatched = 0.
 *   Depth labels (fp32 or fp64 [h][w], stride in ELEMENTS, no crop): mn and mx over the whole plane by numpy's rule -- any NaN makes both NaN;
 *     g = (v - mn) / (mx - mn) in the label's own type, one subtraction and one division, fp64 then rounded to nearest into fp32; sampled by the same
 *     tables (h -> oh, w -> ow).  What numpy answers, this answers: a constant plane gives 0 / 0 = NaN everywhere, a NaN anywhere an all-NaN plane,
 *     infinities follow IEEE; the depth score then reports the frame (nonfinite, nan_frames).  A NaN's sign and payload are not part of the contract.
 *     Among equal extremes -0.0 is the smaller (numpy leaves a zero extreme's sign to its reduction order).  min, max: as double; nonfinite: NaNs and
 *     infinities of the input; n = h * w.
 *   kind: VP_SCENESEG for a colour label, VP_DOMAINSEG for a mask label, VP_SCENE3D for a depth label.
 *   Stated: the nearest rule is the project's reading of resizeNN, unpinned against albumentations / cv2; createGroundTruth, extractROI and the depth
 *     normalisation are pinned (tools/pin_label.py).  The reference's apply_augmentations indexes getItemVal's list in a way that does not run as
 *     written; this follows what it evidently intends: planes background, foreground, road.
 * vp_metric_add_seg_label / vp_metric_add_depth_label: the engines of vp_metric_add_seg / vp_metric_add_depth under the same ordering contract.  The label
 *   lies in host memory and is copied before the call returns.
 * vp_metric_add_seg_logits_label / vp_metric_add_depth_plane_label: the operator forms on a caller's fp32 logits [c][oh][ow] / plane [oh][ow], host or
 *   (on_device != 0) device, as vp_metric_add_seg_logits / vp_metric_add_depth_plane take them.
 * vp_metric_label_frames: label records since the last reset (which empties them).  vp_metric_fetch_labels: waits for the metric's stream and copies the
 *   first min(cap, frames) records.
 * vp_op_label_gt / vp_op_label_depth_gt: the label kernels alone, host in, host out: gt_out [oh][ow] bytes / floats and *frame_out; no engine, no metric.
 * Records are bit-identical from run to run: integer partials, one per workgroup, and the extremes folded in a fixed tree.
 * ERRORS.  VP_ERR_ARG: channels outside {1, 3}; n_colours outside 1 .. 16 or a class above 2 (channels 3); a crop with cw or ch below 1, or a
 *   coordinate outside -16384 .. 32768; h or w outside 1 .. 16384; a stride below the row; an unknown dtype; a null pointer; the refusals of
 *   vp_metric_add_seg / _add_depth / _add_seg_logits / _add_depth_plane.  VP_ERR_STATE: as vp_metric_add_seg.  A refused call adds no record.
 * No call waits for the device beyond the exceptions of vp_metric_add_seg, the first use of a (source, destination) size pair (its table is uploaded
 *   once and kept; the sixteen most recent pairs stay) and the allocation of the label records by the first call. */
enum vp_label_dtype { VP_LABEL_F32 = 0, VP_LABEL_F64 = 1 };
typedef struct vp_label_frame {
  int kind;
  uint32_t n, freq[3], unmatched, outside, nonfinite;
  double min, max;
} vp_label_frame;
/* const uint8_t table[9][4] = VP_SCENESEG_COLOURS_INIT; */
#define VP_SCENESEG_COLOURS_INIT                                                                                                              \
  {{61, 184, 255, 0}, {61, 93, 255, 0}, {216, 255, 61, 0}, {0, 0, 0, 0}, {255, 61, 61, 1}, {255, 190, 61, 1}, {255, 116, 61, 1}, {255, 28, 145, 1}, \
   {0, 255, 220, 2}}
int vp_metric_add_seg_label(vp_metric* m, vp_engine* e, const uint8_t* label, int channels, int h, int w, int stride_bytes, const int* crop_ltrb, const uint8_t* colours,
                            int n_colours);
int vp_metric_add_depth_label(vp_metric* m, vp_engine* e, const void* label, int dtype, int h, int w, int stride_elems);
int vp_metric_add_seg_logits_label(vp_metric* m, const float* logits_chw, int on_device, int c, int oh, int ow, const uint8_t* label, int channels, int h, int w,
                                   int stride_bytes, const int* crop_ltrb, const uint8_t* colours, int n_colours);
int vp_metric_add_depth_plane_label(vp_metric* m, const float* pred, int pred_on_device, int oh, int ow, const void* label, int dtype, int h, int w, int stride_elems);
int vp_metric_label_frames(const vp_metric* m);
int vp_metric_fetch_labels(vp_metric* m, vp_label_frame* records, int cap);
int vp_op_label_gt(int gpu_id, const uint8_t* label, int channels, int h, int w, int stride_bytes, const int* crop_ltrb, const uint8_t* colours, int n_colours, int oh, int ow,
                   uint8_t* gt_out, vp_label_frame* frame_out, char* err, size_t err_len);
int vp_op_label_depth_gt(int gpu_id, const void* label, int dtype, int h, int w, int stride_elems, int oh, int ow, float* gt_out, vp_label_frame* frame_out, char* err,
                         size_t err_len);

/* ---- vp_lanes: the production lane filter on the device, logits in, fits out -----------------------------------------------------------
 * What LaneFilter::update (VisionPilot/production_release/src/lane_filtering/lane_filter.cpp) computes between the EgoLanes pass and
 * LaneTracker: two lane polynomials with their start points and search windows.  A vp_lanes handle owns a stream, a ring of `capacity` device
 * records and the smoothing state.  vp_lanes_add reads an engine's device-resident logits behind its pass, ordered by events alone (the contract
 * of vp_metric_add_seg), queues one kernel and returns; vp_lanes_fetch is the one synchronisation and moves about 1 KB per frame.
 * Geometry: three fp32 planes [3][80][160] -- ego left, ego right, other lanes.  A pixel is SET iff logit > threshold (a NaN is never set).
 *   START POINTS.  Left: rows 79 down to 40, in each row x from 79 down to 0 on the ego-left plane, the first set pixel.  Right: the same rows, x
 *     from 80 up to 159 on the ego-right plane.  No hit: start = (-1, -1), the lane has no windows, points or fit, and its previous fit is forgotten.
 *   SEARCH.  Per lane an upward run from the start point, then a downward run from 4 rows below it; each at most 20 steps.  A step at (x, y): it
 *     ends the run when x is outside 0 .. 159, or y < 0 (up) / y >= 80 (down).  Half-width w = 1 when y < 40, else 6.  The window is columns
 *     [x - w, x + w) and rows [y - 4, y) (up) or [y, y + 4) (down), clipped to the plane; it is recorded as x, y, width, height.  The set pixels of
 *     the lane's own plane in the window, in row-major order, are the ego set; those of the other-lane plane the other set, empty when y < 40.
 *     The ego set is taken when it has 3 pixels or more, else the other set when it has 3 or more.  A taken set is appended to the lane's points
 *     (pixels of overlapping windows appear again); with its float centroid (cx, cy) = (sum x / n, sum y / n), d = (cx - x, cy - y) and
 *     |d| = sqrt(dx dx + dy dy) (fp32, no fused multiply-add), the direction becomes d / |d| when |d| > 0.1f, and (x, y) = (roundf(cx), roundf(cy)).
 *     Nothing taken: an upward run ends when y < 20; either run ends at the 12th empty window in a row; else (x, y) += (int)(direction * 4),
 *     truncated.  The direction starts as (0, -1) / (0, 1).  Last, an upward run at y >= window bottom - 1 moves 4 rows up, a downward run at
 *     y <= window top + 1 moves 4 rows down.
 *   MOMENTS.  Over the lane's points, exact in 64-bit integers: S[k] = sum y^k (k = 0 .. 4), T[k] = sum x y^k (k = 0 .. 2), min_y, max_y.
 *   FIT (vp_lanes_fetch, on the host).  n = S[0] < 4: none.  n < 30: the least-squares line x = b y + c; else the quadratic x = a y^2 + b y + c.
 *     The normal equations are solved by Cramer's rule, every determinant exact in 128-bit integers, each coefficient ONE correctly rounded
 *     quotient.  raw_coeffs = {0, a, b, c, min_y, max_y} (a = 0 for a line), `order` 1 or 2.
 *     DEPARTURE 1: the reference's RANSAC loop (:137-177) is not run.  Its best inlier set starts as all points and is replaced only by a strictly
 *     larger set, and every inlier set is a subset of the points: the final refit is always on all points, the loop only consumes random numbers.
 *     DEPARTURE 2: a singular system (all points on one row; a quadratic's on two rows) gives order 0, VP_LANES_SINGULAR and no coefficients; the
 *     reference's SVD solve would answer the minimum-norm solution.  The previous fit is left as it is, as for n < 4.
 *     NOT PINNED: the reference solves the same least-squares problem with cv::solve(DECOMP_SVD) in double; how far its rounding lies from the
 *     exact solution was not measured (no OpenCV where this was built).  tests/test_lane_filter_host.py measures numpy.linalg.lstsq instead.
 *   SMOOTHING (vp_lanes_fetch, in the order of the adds).  A lane with a fit: when the previous fit is valid all six numbers become
 *     s * raw + (1.0f - s) * previous (s a float, default 0.5f; products and sum in double, VP_LANES_SMOOTHED); the result is `coeffs`,
 *     coeffs_valid = 1, and it is the new previous fit.  A start point but no fit: coeffs_valid = 0, the previous fit untouched.  No start point:
 *     the previous fit is forgotten.  vp_lanes_reset forgets both; it is refused while records are pending.
 * vp_lanes_add: e is a VP_EGOLANES engine (a shared-prefix head included) of output 3 x 80 x 160 with a pass behind it.
 * vp_lanes_add_logits: the operator entry on host floats [3][80][160], copied before the call returns.
 * vp_lanes_fetch: the oldest min(max, pending) records into out, *n their number; they stop being pending.
 * vp_lanes_fetch_points: the point list of lane `lane` (0 left, 1 right) of pending record `record_index` (0 = the oldest, the first the next
 *   vp_lanes_fetch returns): byte pairs (x, y), the upward run's points then the downward run's, at most 1920.  *n = the lane's point count;
 *   min(*n, max_points) pairs are written.  Refused (VP_ERR_STATE) when nothing is pending: a fetch ends a record's window.
 * vp_lanes_fit: the host solve alone, no device, no handle.  out = {a, b, c}; *singular (may be NULL) = 1 and out untouched for a singular
 *   system (still VP_OK).  VP_ERR_ARG: a null pointer, order not 1 or 2, a moment of magnitude 2^40 or more.
 * ERRORS.  VP_ERR_ARG: a null pointer, another engine kind or output size, an engine on another GPU, capacity outside 1 .. 4096, an index or lane
 *   out of range.  VP_ERR_STATE: an engine with no pass yet, `capacity` records pending already, a reset with records pending.  A refused call
 *   changes nothing.  One thread drives a handle. */
#define VP_LANES_MAX_WINDOWS 40
#define VP_LANES_MAX_POINTS 1920
enum vp_lanes_flags { VP_LANES_SINGULAR = 1, VP_LANES_SMOOTHED = 2 };
typedef struct vp_lanes vp_lanes;
typedef struct vp_lanes_lane {
  int32_t start_x, start_y;                      /* (-1, -1): no start point */
  int32_t n_windows_up, n_windows_down;
  int32_t n_points_up, n_points_down;
  int32_t min_y, max_y;                          /* (80, -1) without points */
  int64_t S[5], T[3];
  int16_t windows[VP_LANES_MAX_WINDOWS][4];      /* x, y, width, height; the upward run's first */
  int32_t order, flags, coeffs_valid, reserved;
  double raw_coeffs[6], coeffs[6];
} vp_lanes_lane;
typedef struct vp_lanes_result {
  vp_lanes_lane lane[2];                         /* ego left, ego right */
} vp_lanes_result;
int vp_lanes_create(vp_lanes** out, int gpu_id, int capacity, char* err, size_t err_len);
void vp_lanes_destroy(vp_lanes* l);
const char* vp_lanes_last_error(const vp_lanes* l);
int vp_lanes_set_smoothing(vp_lanes* l, float smoothing);
int vp_lanes_reset(vp_lanes* l);
int vp_lanes_add(vp_lanes* l, vp_engine* e, float threshold);
int vp_lanes_add_logits(vp_lanes* l, const float* logits_3x80x160, float threshold);
int vp_lanes_pending(const vp_lanes* l);
int vp_lanes_fetch(vp_lanes* l, vp_lanes_result* out, int max, int* n);
int vp_lanes_fetch_points(vp_lanes* l, int record_index, int lane, uint8_t* xy, int max_points, int* n);
int vp_lanes_fit(const int64_t S[5], const int64_t T[3], int order, double out[3], int* singular);

/* ---- multi-camera result exchange (BASELINE configs[3]) ---------------------------------------
 * One process (or thread) per GPU, camera r on rank r, weights replicated, no data-path collective in the networks.  For the
 * fused ego-path / BEV consumer every rank needs all cameras' results: ONE ncclAllGather (RCCL over xGMI) per frame of a
 * fixed-size record -- the u8 mask (320x640 = 204.8 KB; EgoLanes label map 80x160 = 12.8 KB) or the fp32 logits (EgoLanes
 * 3x80x160 = 153.6 KB) -- enqueued on the ENGINE's stream behind the frame's graph, no host synchronisation:
 *     rank 0: vp_comm_unique_id(id);  host distributes the 128 bytes (ROS parameter / file / MPI / ...)
 *     all   : vp_comm_create(&c, id, rank, world, gpu, record_bytes_max, ...)
 *     frame : vp_enqueue(e);  vp_gather(e, c, VP_GATHER_MASK);            // overlaps the next in-flight frame's encoder
 *     read  : vp_comm_device_buffer (device consumer) or vp_comm_fetch (host copy, synchronises).
 * RCCL is bound with dlopen at the first vp_comm_* call (librccl.so is not a load-time dependency of libvp_hip.so).
 * One communicator per engine in flight: RCCL operations on one communicator must not run concurrently on two streams -- ENFORCED:
 * vp_gather with an engine on another stream while the communicator's previous all-gather has not completed returns VP_ERR_STATE.
 * The reference has no counterpart (single camera per backend instance). */
typedef struct vp_comm vp_comm;
#define VP_COMM_ID_BYTES 128
enum vp_gather_what { VP_GATHER_MASK = 0, VP_GATHER_LOGITS = 1 };
int vp_comm_unique_id(void* id_out_128, char* err, size_t err_len);
int vp_comm_create(vp_comm** out, const void* unique_id_128, int rank, int world, int gpu_id, size_t record_bytes_max, char* err,
                   size_t err_len);
void vp_comm_destroy(vp_comm* c);
const char* vp_comm_last_error(const vp_comm* c);
int vp_comm_rank(const vp_comm* c);
int vp_comm_world(const vp_comm* c);
int vp_gather(vp_engine* e, vp_comm* c, int what);                              /* async, on the engine's stream */
int vp_comm_device_buffer(const vp_comm* c, void** dev, size_t* record_bytes);  /* [world][record_bytes] */
int vp_comm_fetch(vp_comm* c, vp_engine* e, const void** host, size_t* record_bytes); /* D2H + sync; pinned, valid until next fetch */

/* ---- introspection (profiling, per-layer parity tests) --------------------------------------------------- */
int vp_layer_count(const vp_engine* e);
int vp_layer_info(const vp_engine* e, int i, const char** name, double* flops, double* bytes);
int vp_layer_kernel(const vp_engine* e, int i, const char** kernel_tag);        /* kernel instantiation of launch i */
int vp_layer_launch(const vp_engine* e, int i, const char** launch);            /* its geometry beyond the tag: "nsplit=4", "groups=32", "" */
/* vp_layer_info's flops count the REFERENCE formulation of the layer(s) a launch computes (one multiply-add per product of the
 * reference's operators).  A composed up-sampling stage (round 6: ConvTranspose [+ skip link] -> 3x3 multiplied out at load) executes 0.40-0.51x
 * of that; this returns what the launch executes (= vp_layer_info's figure for every other launch). */
int vp_layer_flops_executed(const vp_engine* e, int i, double* flops);
int vp_profile_layers(vp_engine* e, int iters, float* ms_per_layer, int capacity); /* eager, event per launch */
int vp_tensor_count(const vp_engine* e);
int vp_tensor_info(const vp_engine* e, int i, const char** name, int* c, int* h, int* w);
int vp_tensor_read(vp_engine* e, int i, float* dst_chw);                       /* fp32 CHW copy of an activation */

/* ---- AutoSpeed detector: letterbox preprocess and decode + NMS on the device ------------------------------------
 * Replaces AutoSpeedOnnxEngine::preprocessAutoSpeed (VisionPilot/middleware_recipes/common/backends/autospeed/
 * onnxruntime_engine.cpp:71-113) and ::postProcess / ::computeIoU / ::applyNMS (:170-290); the TensorRT engine (tensorrt_engine.cpp)
 * holds the same two stages.  Two forms:
 *   one call : a VP_AUTOSPEED engine (the detector network on the device, see vp_model_kind) attached with vp_detect_attach, then
 *              vp_detect_infer per frame: letterbox -> network (the engine's replayed graph) -> decode + NMS, no tensor leaves the device;
 *   two calls: the host runs a detector of its own between vp_detect_preprocess and vp_detect_postprocess and hands its output tensor
 *              [num_attrs][num_boxes] (cx, cy, w, h in letterbox pixels, then the class scores) to the latter.
 * vp_detection is the reference's `Detection` (autospeed/detection.hpp:8-12), field for field.  A handle owns its stream and buffers and is
 * not thread-safe (one handle per calling thread, as the reference has one engine object per thread); every call returns synchronised.
 * With raw_on_device the caller's producer must have finished writing the tensor (the call does not wait on foreign streams). */
typedef struct vp_detect vp_detect;
typedef struct vp_detection {
  float x1, y1, x2, y2; /* image coordinates, clamped to the frame */
  float confidence;
  int class_id;         /* -1: no class score was positive (the reference's argmax starts from 0) */
} vp_detection;
/* net_h x net_w: the detector's input (640 x 640); max_boxes <= 16384 and max_attrs >= 5 bound the output tensors accepted later */
int vp_detect_create(vp_detect** out, int gpu_id, int net_h, int net_w, int max_boxes, int max_attrs, char* err, size_t err_len);
void vp_detect_destroy(vp_detect* d);
const char* vp_detect_last_error(const vp_detect* d);
/* BGR8 frame -> [3][net_h][net_w] fp32 planes R, G, B in [0, 1]: resize keeping the aspect (scale = min(net_w / w, net_h / h), new size
 * truncated), centred on a canvas of 114s.  The tensor stays on the device (vp_detect_input_device); dst_host_chw may be NULL.  Remembers
 * the letterbox geometry for the next vp_detect_postprocess (the reference's scale_, pad_x_, pad_y_, orig_width_, orig_height_). */
int vp_detect_preprocess(vp_detect* d, const uint8_t* bgr, int h, int w, int stride_bytes, float* dst_host_chw);
int vp_detect_input_device(const vp_detect* d, void** dev_f32_chw);
int vp_detect_letterbox(const vp_detect* d, float* scale, int* pad_x, int* pad_y);
int vp_detect_set_letterbox(vp_detect* d, float scale, int pad_x, int pad_y, int orig_w, int orig_h); /* geometry from elsewhere */
/* raw: host pointer, or device pointer when raw_on_device != 0.  Per box: strict-'>' argmax of the class scores from 0, `score <
 * conf_thresh` dropped, box back to image coordinates and clamped; then sorted by confidence (descending; equal confidences keep the box
 * order, which the reference's std::sort leaves unspecified) and greedily suppressed per class at IoU > iou_thresh.  *count = detections
 * kept; min(*count, out_cap) of them are written, in the reference's output order. */
int vp_detect_postprocess(vp_detect* d, const float* raw, int raw_on_device, int num_attrs, int num_boxes, float conf_thresh, float iou_thresh,
                          vp_detection* out, int out_cap, int* count);
/* One-call form.  vp_detect_attach: `net` is BORROWED (it must outlive the attachment; NULL detaches).  VP_ERR_ARG unless it is a VP_AUTOSPEED
 * engine on the detector's GPU, the detector was created with net_h x net_w = 512 x 1024, max_boxes >= 10752 and max_attrs >= 4 + nc.
 * vp_detect_infer: frame -> detections, arguments as vp_detect_preprocess + vp_detect_postprocess.  The letterbox kernel writes the engine's input
 * tensor, the engine's graph runs on the engine's stream, decode + NMS read the engine's output tensor in place; the two streams are ordered by
 * events and the call waits for the device ONCE, at its end (the wait ahead of the frame's staging copy finds the detector's stream drained, since every
 * call -- a failing one included -- returns with both streams drained; a frame of a new size uploads its tap tables and waits for them, once per size;
 * a handle's first call also runs the engine's eager warm-up pass).  A
 * non-finite network output (vp_set_finite_check on the engine, default on) returns VP_ERR_RANGE.  The raw tensor of the frame stays readable
 * through vp_logits(net). */
int vp_detect_attach(vp_detect* d, vp_engine* net);
int vp_detect_infer(vp_detect* d, const uint8_t* bgr, int h, int w, int stride_bytes, float conf_thresh, float iou_thresh, vp_detection* out,
                    int out_cap, int* count);
/* vp_detect_infer on the region (x0, y0, w, h; all four 0: the whole frame) of a device-resident vp_frame (above): the detector's stream waits for
 * the frame's content and copies the region device to device into its frame buffer; no staging copy, no H2D; everything behind is vp_detect_infer.
 * VP_ERR_ARG for a frame on another GPU or a bad region, VP_ERR_STATE for a frame never uploaded. */
int vp_detect_infer_frame(vp_detect* d, vp_frame* f, int x0, int y0, int w, int h, float conf_thresh, float iou_thresh, vp_detection* out, int out_cap,
                          int* count);
/* The same stages in the arithmetic of the PYTHON wrapper, Models/inference/auto_speed_infer.py AutoSpeedNetworkInfer, which no thresholds of the
 * entries above reproduce (infer.AutoSpeedNetworkInfer is built on these; they share the handle, its buffers and its stored geometry with them):
 *   vp_detect_preprocess_pil  resize_letterbox + ToTensor (:24-42): scale = min(net_w / w, net_h / h) in double, new size int(w * scale), Pillow's
 *       antialiased Image.BILINEAR resize bit for bit (the tables of vp_resample_coeffs, u8 between the horizontal and the vertical pass), pasted at
 *       pad = (net - new) / 2 on a canvas of 114s, planes R, G, B of u8 / 255 (one fp32 division).  pixel_format: VP_RGB8 (a PIL image) or VP_BGR8.
 *       The geometry is stored for the decode and reported by vp_detect_letterbox (scale rounded to float).
 *   vp_detect_postprocess_agnostic  post_process_predictions + the back-mapping (:63-83, :100-106): score = max over the classes of
 *       sigmoid(raw score), class = the first maximum, `score > conf_thresh` kept; corners cx -+ w / 2; greedy suppression by descending score
 *       (equal scores in box order) at IoU > iou_thresh WHATEVER the classes, IoU = inter / (a + b - inter) in letterbox pixels (the
 *       torchvision.ops.nms rule); kept boxes -> (x - pad) / scale, clamped to the frame.  out_rows6: [out_cap][6] floats x1, y1, x2, y2, score,
 *       class; *count and out_cap as vp_detect_postprocess.
 *   vp_detect_infer_pil  both around the attached network: the streams, events and the one wait of vp_detect_infer; VP_ERR_RANGE likewise.
 * vp_detect_geometry_pil (host only): the letterbox geometry alone; VP_ERR_ARG when the resized image would be empty. */
int vp_detect_geometry_pil(int net_h, int net_w, int h, int w, double* scale, int* new_w, int* new_h, int* pad_x, int* pad_y);
int vp_detect_preprocess_pil(vp_detect* d, const uint8_t* frame, int h, int w, int stride_bytes, int pixel_format, float* dst_host_chw);
int vp_detect_postprocess_agnostic(vp_detect* d, const float* raw, int raw_on_device, int num_attrs, int num_boxes, float conf_thresh, float iou_thresh,
                                   float* out_rows6, int out_cap, int* count);
int vp_detect_infer_pil(vp_detect* d, const uint8_t* frame, int h, int w, int stride_bytes, int pixel_format, float conf_thresh, float iou_thresh,
                        float* out_rows6, int out_cap, int* count);

/* ---- single-operator entries of the detector network's kernels (unit tests; not used by callers) -----------
 * vp_op_detect_head_decode: box [3 levels one after the other][64][h_l][w_l] and cls [..][nc][h_l][w_l] fp32 CHW logits, level l of size
 *   (h0 >> l) x (w0 >> l), stride 8 << l -> out [4 + nc][sum h_l w_l] (AutoSpeedHead.forward in eval mode behind the convolutions).
 * vp_op_upsample2_cat: a [ca][h][w], b [cb][2h][2w] -> out [ca + cb][2h][2w] = cat(nearest x2 of a, b); the (hi, lo) planes the kernel moves are
 *   returned as they are: out_hi / out_lo are uint16 fp16 bit patterns [ca + cb][2h][2w] (out_lo all zero for VP_FP16).
 * vp_op_dwconv3x3: depthwise 3x3 (pad 1) + bias + activation (ActFn code: 0 none, 2 SiLU) [+ add]: in [c][h][w], weight [c][3][3], add NULL or
 *   [c][h][w] -> out_hi / out_lo as above. */
int vp_op_detect_head_decode(int gpu_id, int precision, const float* box, const float* cls, int nc, int h0, int w0, float* out, char* err, size_t err_len);
int vp_op_upsample2_cat(int gpu_id, int precision, const float* a, int ca, const float* b, int cb, int h, int w, uint16_t* out_hi, uint16_t* out_lo,
                        char* err, size_t err_len);
int vp_op_dwconv3x3(int gpu_id, int precision, const float* in, int c, int h, int w, const float* weight, const float* bias, int act, const float* add,
                    uint16_t* out_hi, uint16_t* out_lo, char* err, size_t err_len);
/* ---- single-operator entries of the activation-scale mechanism (unit tests; not used by callers) ------------
 * vp_op_absmax: act_absmax_kernel on (hi, lo) fp16 bit patterns laid out [h][w][c_pitch] (lo may be NULL): max |hi + lo| over the channels [0, c) of
 *   every pixel, non-finite elements left out and counted in *nonfinite.
 * vp_op_conv2d_scaled: vp_op_conv2d (mode 0) with the input stored as in * 2^-in_exp, the residual as res * 2^-res_exp and the result as
 *   y * 2^-out_exp; in / res are TRUE values (scaled on the host); out_hi / out_lo are the STORED planes, fp16 bit patterns [cout][h][w]. */
int vp_op_absmax(int gpu_id, const uint16_t* hi, const uint16_t* lo, int c, int h, int w, int c_pitch, float* absmax, unsigned* nonfinite, char* err,
                 size_t err_len);
int vp_op_conv2d_scaled(int gpu_id, int precision, int mode, const float* in, int cin, int h, int w, const float* weight, const float* bias, int cout,
                        int ks, int act, int res_mode, const float* res, int tile, int bk, int nsplit, int in_exp, int res_exp, int out_exp,
                        uint16_t* out_hi, uint16_t* out_lo, char* err, size_t err_len);
/* vp_op_exp_hist: act_exp_hist_kernel (the range survey's histogram) on planes laid out as for vp_op_absmax: bins[VP_RANGE_BINS], *zeros and *count as
 *   in vp_range_stats.  A finite |hi + lo| of 2^16 or more (no pair an engine stores) is counted in the top bin. */
int vp_op_exp_hist(int gpu_id, const uint16_t* hi, const uint16_t* lo, int c, int h, int w, int c_pitch, unsigned long long* bins,
                   unsigned long long* zeros, unsigned long long* count, char* err, size_t err_len);
/* ---- single-operator entries of the AutoSteer head's kernels (unit tests; not used by callers) ------------
 * vp_op_rowpair_conv: Conv2d(cin -> 32, kernel (2,1), stride (2,1)) + bias + SiLU: in [cin][h][w], weight [32][cin][2][1], bias [32].  The result,
 *   (h / 2) x w -- with replicate every pixel stored 2 x 2: h' x 2w, h' = 2 (h / 2) -- lands in channels [dst_off, dst_off + 32) of a destination of dst_c channels
 *   (multiples of 32) that starts as dst_init ([dst_c][h'][w'] or NULL = zeros); out_hi / out_lo: the whole destination as fp16 bit patterns.
 * vp_op_lane_rows_head: features [cin][h][256] -> out [2][h] (xp, h_vector): c1_w / c2_w [cin][3][3] and c1_b / c2_b with the BatchNorm folded in,
 *   h1_w / h2_w [16]. */
int vp_op_rowpair_conv(int gpu_id, int precision, const float* in, int cin, int h, int w, const float* weight, const float* bias, int replicate,
                       int dst_c, int dst_off, const float* dst_init, uint16_t* out_hi, uint16_t* out_lo, char* err, size_t err_len);
int vp_op_lane_rows_head(int gpu_id, int precision, const float* features, int cin, int h, int w, const float* c1_w, float c1_b, const float* c2_w,
                         float c2_b, const float* h1_w, float h1_b, const float* h2_w, float h2_b, float* out_2xh, char* err, size_t err_len);
/* ---- the detector's and the lane network's own kernels under the activation scale (unit tests; not used by callers) ------------
 * The float arguments are TRUE values; the entry stores them as x * 2^-exp (scaled on the host: exact) and hands the exponents to the launch.  With every
 * exponent 0 a launch is the one of the entry without the suffix: same parameter block, same bits.
 * vp_op_upsample2_cat_scaled: channels [a_off, a_off + a_nch) of a [ca][h][w] and [b_off, b_off + b_nch) of b [cb][2h][2w] (multiples of 8) in an engine
 *   created with VP_ACT_SCALE, which ties a, b and the result to ONE exponent; out_hi / out_lo: the STORED planes [a_nch + b_nch][2h][2w].
 * vp_op_detect_head_decode_scaled: exps[6] = (box, cls) exponents of the three levels; out is true-valued like vp_op_detect_head_decode's.
 * vp_op_rowpair_conv_scaled: in stored under in_exp, the whole destination (dst_init included) under out_exp; out_hi / out_lo: the STORED planes.
 * vp_op_lane_rows_head_scaled: features stored under in_exp; out_2xh is true-valued. */
int vp_op_upsample2_cat_scaled(int gpu_id, int precision, const float* a, int ca, int a_off, int a_nch, const float* b, int cb, int b_off, int b_nch, int h,
                               int w, int exp, uint16_t* out_hi, uint16_t* out_lo, char* err, size_t err_len);
int vp_op_detect_head_decode_scaled(int gpu_id, int precision, const float* box, const float* cls, int nc, int h0, int w0, const int* exps, float* out,
                                    char* err, size_t err_len);
int vp_op_rowpair_conv_scaled(int gpu_id, int precision, const float* in, int cin, int h, int w, const float* weight, const float* bias, int replicate,
                              int dst_c, int dst_off, const float* dst_init, int in_exp, int out_exp, uint16_t* out_hi, uint16_t* out_lo, char* err,
                              size_t err_len);
int vp_op_lane_rows_head_scaled(int gpu_id, int precision, const float* features, int cin, int h, int w, const float* c1_w, float c1_b, const float* c2_w,
                                float c2_b, const float* h1_w, float h1_b, const float* h2_w, float h2_b, int in_exp, float* out_2xh, char* err,
                                size_t err_len);

/* ---- the e4m3 MFMA layer of VP_MFMA_FP8 engines (unit tests; not used by callers) ------------
 * vp_op_conv3x3_f8: Conv2d 3x3 (stride 1, pad 1) + bias + act (0 none, 1 GELU) on conv3x3_f8_kernel under the activation exponent qexp (FP8 MFMA
 *   ENGINES above) -- the engine's own packer and launch, whatever the map size.  in [cin][h][w] fp32 (rounded to fp16 first, as an engine stores it),
 *   weight [cout][cin][3][3], bias [cout]; out_f16: the stored fp16 bit patterns [cout][h][w].  VP_ERR_ARG unless cin and cout, each rounded up to 32 as an engine
 *   pads them, are multiples of 64 and the map is at least 8 x 16 pixels.
 * vp_op_fp8_quantize: the kernel's quantiser (a device function) over an array of n fp16 bit patterns; equals vp_fp8_quantize_act bit for bit. */
int vp_op_conv3x3_f8(int gpu_id, const float* in, int cin, int h, int w, const float* weight, const float* bias, int cout, int act, int qexp,
                     uint16_t* out_f16, char* err, size_t err_len);
int vp_op_fp8_quantize(int gpu_id, const uint16_t* f16, size_t n, int qexp, uint8_t* codes, char* err, size_t err_len);

/* ---- the convolution forms the networks launch beyond vp_op_conv2d's (unit tests; not used by callers) ------------
 * vp_op_conv2d_forms: Conv2d ks x ks (pad ks / 2, stride 1 or 2: stride 2 needs ks == 3 and even h, w) + bias + act, then the residual (res_mode
 *   1: y + r, 2: y * r + r, applied BEHIND the activation), then post_act -- through the engine's own add_conv, so dispatch, weight packing and
 *   epilogue routing are the production ones.  in [cin][h][w], weight [cout][cin][ks][ks], bias [cout] fp32; precision may carry VP_WEIGHTS_FP8.
 *   Destination: dst_c == 0: a fresh [cout][oh][ow] tensor (oh = h / stride).  Else a dst_c-channel tensor that starts as dst_init ([dst_c][oh][ow];
 *   NULL = zeros), and the launch stores through an alias view of its channels [dst_off, dst_off + cout) (dst_c, dst_off, cout: multiples of 32).
 *   Residual (res_mode != 0): res_where 0: a fresh tensor uploaded from res [cout][res_h][res_w] (res_h / res_w 0 = the output's size; any other size
 *   is refused when the plan is built); res_where 1: channels [res_off, res_off + cout) of the destination tensor itself, values from dst_init.
 *   Input: in_c == 0: a fresh [cin][h][w] tensor; else an alias view of channels [in_off, in_off + cin) of an in_c-channel tensor (refused when the
 *   plan is built: a convolution's input cannot be a slice).
 *   Exponents: all 0: an unflagged engine (unless precision itself carries VP_ACT_SCALE).  Else an engine with VP_ACT_SCALE: in / res / dst_init are TRUE values, stored as x * 2^-exp (scaled on
 *   the host: exact) under in_exp / res_exp / out_exp; a slice shares its tensor's exponent, so with res_where 1 the residual is stored under
 *   out_exp and res_exp is not read.
 *   out_hi / out_lo: the STORED planes of the WHOLE destination tensor, fp16 bit patterns [dst_c or cout][oh][ow] (out_lo all zero for VP_FP16). */
typedef struct vp_conv_form {
  int cin, h, w, cout, ks, stride;
  int act, post_act, res_mode;            /* ActFn / residual codes as vp_op_conv2d */
  int tile, bk, nsplit;                   /* -1 = the dispatch rule */
  int dst_c, dst_off;
  int res_where, res_off, res_h, res_w;
  int in_c, in_off;
  int in_exp, res_exp, out_exp;
} vp_conv_form;
int vp_op_conv2d_forms(int gpu_id, int precision, const vp_conv_form* form, const float* in, const float* weight, const float* bias, const float* res,
                       const float* dst_init, uint16_t* out_hi, uint16_t* out_lo, char* err, size_t err_len);

/* ---- single-operator entry (unit parity tests of the MFMA conv kernel; not used by callers) -------------- */
/* mode 0: Conv2d k=ks stride 1 pad ks/2, weight [Cout][Cin][ks][ks]; mode 1: ConvTranspose2d k2 s2, weight
 * [Cin][Cout][2][2].  act: 0 none 1 GELU 2 SiLU.  res_mode: 0 none 1 add 2 mul-add; res has the output shape.
 * mode 2: ConvTranspose2d k2 s2 of `in` + Conv2d 1x1 of a skip tensor in ONE launch (the decoders' up-sample + skip-link
 * pairs): `res` is the skip INPUT [res_mode channels][2h][2w], weight = ConvTranspose weight followed by the 1x1 weight
 * [Cout][res_mode], bias = the two bias vectors one after the other; act / tile / bk / nsplit are ignored.
 * mode 3: a head's last convolution (3x3, no activation): the kernel writes fp32 NCHW logits itself.
 * tile/bk/nsplit: -1 = engine heuristic.  in/res/out are fp32 CHW host buffers. */
int vp_op_conv2d(int gpu_id, int precision, int mode, const float* in, int cin, int h, int w, const float* weight, const float* bias,
                 int cout, int ks, int act, int res_mode, const float* res, int tile, int bk, int nsplit, float* out,
                 char* err, size_t err_len);

/* ---- composed up-sampling stage (round 6; unit parity tests, not used by callers) --------------------------
 * The decoders apply ConvTranspose2d(k2, s2) [+ Conv2d 1x1 of a skip tensor] and then Conv2d 3x3 with NO nonlinearity in between
 * (Models/model_components/scene_neck.py:29-35,41-46,52-57; scene_seg_head.py:24-29,35-38; scene_3d_head.py:26-31,38-41): one linear map.
 * The engine multiplies the three weight sets out at load (fp64 accumulation) and runs the stage as ONE launch on the LOW-resolution
 * tensor: per output phase (Y & 1, X & 1) a 2x2 convolution of it, a 3x3 convolution of the skip tensor with pre-multiplied weights,
 * and a bias that depends only on which high-resolution taps lie inside the map -- 0.40-0.51x the matrix work, same result.
 * vp_compose_upconv: the composition alone.  wt [cin][cm][2][2], bt [cm] (ConvTranspose2d); ws [cm][cs], bs [cm] (1x1 skip link; cs = 0:
 *   none, ws / bs / wsk may be NULL); w3 [cout][cm][3][3], b3 [cout].  Results (fp64):
 *   wx [4 phases py*2+px][4 taps a*2+b][cout][cin]: out(2y+py, 2x+px) += wx . x(y+py-1+a, x+px-1+b) (zero outside the low-resolution map);
 *   wsk [9 taps ty*3+tx][cout][cs]: plain 3x3 / pad 1 convolution of the skip tensor;
 *   bias [9 classes rc*3+cc][cout]: rc / cc = 0 first, 1 inner, 2 last row / column of the OUTPUT map.
 * vp_op_upconv: the whole stage through the engine's kernel: in [cin][h][w], skip [cs][2h][2w] -> out [cout][2h][2w], fp32 CHW host
 *   buffers; act 0 none, 1 GELU; shape 6 / 7 or -1 (dispatch rule); nsplit K slices or 0 (dispatch rule); precision VP_FP16X3 (parity mode) or
 *   VP_FP16 (the fp16 engines' form: 64-channel chunks, one MFMA per product; input channels a multiple of 64 after padding). */
int vp_compose_upconv(int gpu_id, const float* wt, const float* bt, const float* ws, const float* bs, const float* w3, const float* b3, int cin, int cm,
                      int cout, int cs, double* wx, double* wsk, double* bias, char* err, size_t err_len);
int vp_op_upconv(int gpu_id, const float* in, int cin, int h, int w, const float* skip, int cs, const float* wt, const float* bt, const float* ws,
                 const float* bs, const float* w3, const float* b3, int cm, int cout, int act, int shape, int nsplit, int precision, float* out,
                 char* err, size_t err_len);

/* ---- single-operator entry of vp_frame's rectification kernel (unit tests; not used by callers) ------------
 * vp_op_remap_bgr8: frame_remap_kernel on a host BGR8 picture src [src_h][src_w][3] (rows src_stride >= 3 * src_w bytes apart) through ANY map in the
 * exchange form of vp_rectify_map (xy [out_h * out_w][2] int16, frac [out_h * out_w] uint16 = fy << 5 | fx, both below 32) with either vp_border.
 * dst [out_h][out_w][3], rows dst_stride >= 3 * out_w bytes apart; a dst_stride of at least 12 * ceil(out_w / 4) also receives the bytes the kernel
 * writes behind each row's end (zeros).  The device destination is filled with 0xFF before the launch.  Sizes 1 .. 16384 each way. */
int vp_op_remap_bgr8(int gpu_id, const uint8_t* src, int src_h, int src_w, int src_stride, const int16_t* xy, const uint16_t* frac, int out_h, int out_w,
                     int border, uint8_t* dst, int dst_stride, char* err, size_t err_len);
/* vp_op_jpeg_encode_bgr8: the encoder of vp_canvas_fetch_jpeg (vp_canvas, "THE PICTURE AS A BASELINE JPEG") on a host BGR8 picture bgr [h][w][3], rows
 * stride >= 3 * w bytes apart; needs no frame and no canvas.  The stream into dst [cap], its length in *n; refusals and the cap rule as there, the text in
 * err. */
int vp_op_jpeg_encode_bgr8(int gpu_id, const uint8_t* bgr, int h, int w, int stride, int quality, int restart_mcus, uint8_t* dst, size_t cap, size_t* n,
                           char* err, size_t err_len);

/* ---- developer options ------------------------------------------------------------------------------------
 * The library NEVER reads the environment.  The dispatch rules' developer knobs (A/B timing of a kernel against the one it replaced,
 * tile / split-K sweeps: DESIGN.md section 3, csrc/options.cpp for the key list) are set here, process-wide, and affect engines
 * created AFTERWARDS; value NULL removes a key; an unknown key is VP_ERR_ARG.  No option is needed in production and none changes a
 * result beyond fp32 summation order.  vp_version() lists every option in force; vp_plan_hash() = FNV-1a over (launch name, kernel
 * tag, launch geometry) of an engine's plan, so a host (bench.py does) can record exactly which kernels ran.
 * "VP_PLAN_TARGET" = "latency" | "throughput" (anything else: VP_ERR_ARG) selects the kernel plan target for EVERY engine created while it is set --
 * a developer knob for A/B runs since round 6; hosts choose per engine with the creation flag VP_PLAN_LATENCY (vp_precision). */
int vp_set_option(const char* key, const char* value);
const char* vp_get_option(const char* key);       /* NULL when unset */
void vp_clear_options(void);
unsigned long long vp_plan_hash(const vp_engine* e);
/* Device bytes of an engine's matrix / FC WEIGHT tensors by storage class: OCP e4m3 codes (VP_WEIGHTS_FP8 on the kernels that convert on
 * the fly), fp16 planes ((hi, lo) pairs in the parity mode), fp32 (FC rows, the fused MBConv projection / depthwise filters).  Bias and
 * scale vectors, tables and activations are not counted.  Any pointer may be NULL. */
int vp_weight_bytes(const vp_engine* e, unsigned long long* fp8_bytes, unsigned long long* fp16_bytes, unsigned long long* fp32_bytes);
/* host only (tests / external checks): the (hi, lo) fp16 planes the engine makes of a weight matrix [rows][per_row] and the per-row
 * 2^-s of its power-of-two prescale: fp32(hi) + fp32(lo) = w * 2^s with the row maximum in [2^13, 2^14), post_scale[r] = 2^-s.
 * VP_ERR_RANGE for a weight beyond the fp16 range, as vp_create*. */
int vp_split_weight_rows(const float* w, int rows, int per_row, uint16_t* hi, uint16_t* lo, float* post_scale);
/* host only (tests): what VP_WEIGHTS_FP8 storage keeps of a weight matrix -- one OCP e4m3 code per element and the per-row scale
 * (row maximum / 448); for rows that came out of the per-row quantiser (possibly re-scaled since, as BatchNorm folding does)
 * code x scale reproduces the value to fp32 rounding. */
int vp_fp8_encode_rows(const float* w, int rows, int per_row, uint8_t* codes, float* row_scale);

const char* vp_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VP_HIP_H_ */

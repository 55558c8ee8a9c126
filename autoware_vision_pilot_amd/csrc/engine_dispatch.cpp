// libvp_hip engine, part 2 of 3: the DISPATCH RULES -- which kernel, tile and split factor every convolution of a plan gets (choose_conv and its
// family: free functions of the layer's shape and the developer options, callable without an engine), the weight packing that kernel expects
// (pack_index / pack_weight_rows) and the emission of the launch (Engine::push_conv_op).  Every rule here is a measured choice (the comment at the rule
// names the profile); the outcome for every layer of every network is pinned by tests/golden/kernel_plan*.json, and under every developer option by
// tests/golden/plan_options.json (tests/test_engine_emulated.py).
#include "engine_internal.hpp"

namespace vp {

// Round 5: the dispatch rules trade a layer's OWN latency for CU-time where the rest of the frame can use the freed CUs (decode_layer_5 on 100
// workgroups, the neck's map layers on half the workgroups, the K = 288 ConvTranspose on 128) -- right for a camera with forked heads and for several
// cameras per GPU, the configurations bench.py measures; a host that runs ONE network on ONE camera, one frame at a time, has nothing to put on the
// freed CUs and pays 3-7 % of its frame (SceneSeg alone 1.79 -> 1.91 ms).  The creation flag VP_PLAN_LATENCY (round 6: per ENGINE, OR-ed into vp_create's
// precision argument) selects the round-4 choices for that engine; the developer option VP_PLAN_TARGET=latency does it for every engine created while it
// is set (A/B runs of bench.py).  Either way the choice changes vp_plan_hash().  Default / "throughput": the rules above.
bool Engine::plan_latency() const { return (precision_ & 32) != 0 || dev_option_is("VP_PLAN_TARGET", 'l'); }

// Developer option VP_PLAN_OVERRIDE = "<layer>=<tile>[:<nsplit>];<layer>=..." (round 6, tools/plan_search.py): ONE layer's kernel choice, by name --
// <layer> matches a launch whose name ENDS with it ("decode_layer_5" = that layer of every network created while the option is set), <tile> is the
// halo-tile number of a 3x3 convolution (1 / 3: halo kernel 128 / 64 channels, 6 / 7 / 8: pipelined shapes, 11 / 12: map kernels) or the shape (6 / 7)
// of a composed up-sampling stage, <nsplit> its K slices (absent / 0: the rule's).  The in-frame tuner flips single layers with it; the rules below
// are what its table (profiles/r06_plan_search.tsv) says.  Part of the plan hash like every option.
bool plan_override(const std::string& name, int* tile, int* nsplit) {
  const char* e = dev_option("VP_PLAN_OVERRIDE");
  if (!e) return false;
  const std::string s(e);
  size_t pos = 0;
  while (pos < s.size()) {
    size_t end = s.find(';', pos);
    if (end == std::string::npos) end = s.size();
    const std::string item = s.substr(pos, end - pos);
    pos = end + 1;
    const size_t eq = item.rfind('=');
    if (eq == std::string::npos || eq == 0) continue;
    const std::string key = item.substr(0, eq), val = item.substr(eq + 1);
    if (name.size() < key.size() || name.compare(name.size() - key.size(), key.size(), key) != 0) continue;
    const size_t colon = val.find(':');
    *tile = std::atoi(val.substr(0, colon).c_str());
    *nsplit = colon == std::string::npos ? 0 : std::atoi(val.substr(colon + 1).c_str());
    return true;
  }
  return false;
}

// ------------------------------------------------------------------------------------------- conv planning
namespace {

long long cdiv(long long a, long long b) { return (a + b - 1) / b; }
// conv + bias + {GELU, none}: the epilogue the pipelined kernels carry without split-K
bool plain_epilogue(const ConvQuery& q) { return (q.act == ACT_GELU || q.act == ACT_NONE) && q.res_mode == RES_NONE && q.post_act == ACT_NONE; }
int option_int(const char* key, int dflt) {
  const char* e = dev_option(key);
  return e ? std::atoi(e) : dflt;
}

}  // namespace

ConvChoice choose_gemm_cfg(int M, int ncols, int cin_pad, int ks, int forced_tile, int forced_bk, int forced_nsplit) {
  ConvChoice c;
  int tile;
  if (forced_tile >= 0) {
    tile = forced_tile;
  } else if (ncols <= 32) {
    tile = 3;
  } else if (ncols % 128 == 0 && (cdiv(M, 128) * (ncols / 128) >= 192 || (M <= 256 && ncols >= 2048))) {
    tile = 0;  // second case: weight-dominated GEMMs on tiny maps (first up-sampling stage: 200 pixels x 5120 rows): 29 vs 36 us
  } else if (cdiv(M, 128) * cdiv(ncols, 64) >= 128 || M >= 2048) {
    tile = 1;
  } else {
    tile = 2;
  }
  c.tile = tile;
  c.layout = tile == 6 ? GEMM_DMA : GEMM_ROWS;
  c.bk = forced_bk > 0 ? forced_bk : 64;  // 128-byte rows per load, half the K steps of BK=32
  if (cin_pad % c.bk != 0) c.bk = 32;
  c.CoutW = round_up(ncols, conv_tile_co(tile));
  const long long blocks = cdiv(M, conv_tile_px(tile)) * (c.CoutW / conv_tile_co(tile));
  const int S = ks * ks * (cin_pad / c.bk);
  int ns = 1;
  if (forced_nsplit > 0) {
    ns = forced_nsplit;
  } else if (blocks < 128 && S >= 32) {  // split-K pays only for long K loops: it costs a second (finish) launch
    ns = (int)std::min<long long>(cdiv(384, blocks), std::max(1, S / 8));
    ns = std::max(1, std::min(ns, 32));
  } else if (ks == 1 && blocks < 64) {
    // long-K 1x1 GEMMs on small maps (the MBConv projections of stages 4-7: K = 480..1152 on 200-800 pixels, 12-42 workgroups
    // walking 8-18 dependent staging steps): slices of >= 3 steps up to ~128 workgroups.  Measured (parity mode, per launch incl.
    // the finish kernel): 25 -> 15 us on stages 6 / 7, 20 -> 15 on stage 5, SceneSeg single stream 2.076 -> 2.015 ms.
    // VP_PROJ_SPLIT = minimum steps per slice (0 = never split).
    const int min_steps = option_int("VP_PROJ_SPLIT", 3);
    if (min_steps > 0 && S >= 2 * min_steps) ns = std::max(1, std::min<int>(S / min_steps, (int)cdiv(128, blocks)));
  }
  c.nsplit = std::min(ns, std::max(1, S));
  return c;
}

namespace {

// ---- the halo tile of a 3x3 stride-1 convolution, step by step (choose_conv runs them in this order)

// step 1, the base halo rule: LDS-resident halo kernel (kernels_conv3x3.hip) unless overridden (tile >= 100 selects a halo tile); -1 = the generic kernel
int base_halo_tile(const ConvQuery& q, int ncols) {
  int halo = -1;
  const char* env = dev_option("VP_CONV3X3");
  const bool force_v1 = (env && std::strcmp(env, "v1") == 0) || (q.tile >= 0 && q.tile < 100);
  if (q.tile >= 100) {
    halo = q.tile - 100;
  } else if (!force_v1) {
    const long long t256 = cdiv(q.H, 16) * cdiv(q.W, 16), t128 = cdiv(q.H, 8) * cdiv(q.W, 16);
    if (ncols <= 32) {
      halo = (dev_option("VP_HEAD_TILE5") && t256 >= 400) ? 5 : 4;
    } else if (ncols % 128 != 0) {
      halo = (!q.split && t256 * cdiv(ncols, 64) >= 400) ? 2 : 3;
    } else {
      halo = (!q.split && t256 * (ncols / 128) >= 400) ? 0 : 1;
      // fewer 128-channel tiles than CUs: 64-channel tiles double the workgroup count, so the layer needs no split-K
      // (decode_layer_5: 46 us vs 57 us with a 3-way split) or half the split factor and half the fp32 partial
      // traffic (neck layers at 20x40 / 40x80: -1..-5 us each; profiles/r01_splitk_ablation.txt)
      if (halo == 1 && t128 * (ncols / 128) < 256) halo = 3;
    }
  }
  if (halo >= 0 && q.split && (halo == 0 || halo == 2)) halo += 1;
  return halo;
}

// step 2, the pipelined shapes.  *rule_nsplit: the K slices a rule picks TOGETHER with its tile (0 = none)
// parity mode, 128-channel tiles: the pipelined kernels of kernels_conv3x3_x3.hip -- halo tile 7 (8x16 patches, two
// independent workgroups per CU; also the split-K shape of the small-map layers) or 6 (16x16 patches, one 8-wave workgroup)
int pipelined_tile(const ConvQuery& q, int ncols, int halo, int* rule_nsplit) {
  const char* envx = dev_option("VP_X3_TILE");  // developer knob: 0 = halo kernel, 6 / 7 = force that shape
  const long long wgs16 = cdiv(q.H, 16) * cdiv(q.W, 16) * (ncols / 128);
  // measured per layer (profiles/r02_layers_*): the 4-wave shape wins where the K loop is short (Cin <= 128: prologue and
  // epilogue weigh most and two independent workgroups per CU overlap them), the 8-wave shape elsewhere (half the weight
  // staging per MFMA)
  const int want = envx ? std::atoi(envx) : (q.cin_pad <= 128 ? 7 : 6);
  const bool plain = plain_epilogue(q);
  // round 4: the VP_FP16 engines take the same shapes on 64-channel chunks (X1: the planes are the chunk's halves) for their big layers --
  // the halo kernel's lone-wave schedule left them at 0.29-0.31 of peak.  VP_F16_BIG=0 (developer knob, A/B timing): the halo kernel.
  const char* envf = dev_option("VP_F16_BIG");
  if (!q.split && !q.fp8_storage && q.tile < 0 && !(envf && envf[0] == '0') && halo >= 0 && halo <= 3 && ncols % 128 == 0 && q.cin_pad % 64 == 0 && !q.logits_out &&
      !q.in2 && plain && wgs16 >= option_int("VP_F16_MIN_WGS", q.plan_latency ? 160 : 36)) {
    // measured per layer (profiles/r04_layers_sceneseg_fp16_big_ab.tsv): the 8-wave shape wins where ONE round of its workgroups covers the
    // map and the K loop is long (decode_layer_4: 79.6 -> 68.9 us, decode_layer_7: 45.6 -> 40.9); with two rounds (decode_layer_6: 75.6 ->
    // 77.2) or two chunks per workgroup (decode_layer_8: 85.8 -> 95.6 / 83.7 on the 4-wave shape) the halo kernel's two workgroups per CU
    // do as well or better.  VP_F16_BIG=6 / 7 forces a shape on every eligible layer.
    // Round 6, throughput plan: the in-frame search (tools/plan_search.py --precision fp16, profiles/r06_plan_search_fp16.tsv) moves the smaller layers
    // onto the pipelined shapes as well, as round 5 did for the parity mode -- fewer, fatter workgroups leave CUs to the other cameras: decode_layer_5
    // (100 tiles of 16x16 x 128 channels) and decode_layer_3 (60) on the 8-wave shape (+0.5 % / +1.1 % frames/s on the metric pair), decode_layer_1
    // (20x40 map, 36 tiles) on the 4-wave shape in four K slices (+0.6 %); together 1040 -> 1067 frames/s.  The latency plan keeps the 160-tile floor.
    if (envf) halo = std::atoi(envf) == 6 ? 6 : 7;
    else if (wgs16 <= 256 && q.cin_pad >= 256 && wgs16 >= 60) halo = 6;
    else if (wgs16 < 60 && q.cin_pad >= 256 && q.H * q.W <= 800 && q.nsplit <= 0) {
      halo = 7;
      *rule_nsplit = 4;
    }
  }
  if (q.split && q.tile < 0 && want != 0 && (halo == 1 || halo == 3) && ncols % 128 == 0 && !q.logits_out && !q.in2) {
    // Smaller layers stay on the halo kernel's 64-channel tiles (two workgroups per CU, twice the workgroup count): measured
    // on MI355X, the 4-wave shape without split-K took 139 vs 100 us on decode_layer_5 (200 patches) and its split-K form
    // (kernel support kept, tile 107 + nsplit) 63 vs 47 / 79 vs 70 us on decode_layer_1 / 3 (profiles/r02_splitk_x3w4.txt)
    // Round 5: the floor is 100 tiles of 16x16 x 128 channels (it was 160): decode_layer_5 (512 -> 256 on 80x160: exactly 100) moves from the halo kernel's
    // 400 64-channel workgroups to 100 8-wave workgroups of the pipelined shape.  ALONE the layer is slower (101 -> 138 us: 100 CUs), per occupied CU
    // it runs at 2.2 TFLOP/s against 1.16 -- 100 CUs do not pull the package to its power limit -- and with the other head or the other cameras on
    // the remaining CUs the frame rate gains 1.5-3 % at an unchanged one-camera p50 (profiles/r05_dec5_x3w8_ab.txt).  Below 100 (the 40x80 / 20x40
    // maps: 60 / 36 workgroups) the same move LOSES 2 % / 11 %: their launches get 2-4x longer than the rest of the frame can cover.
    // VP_X3_MIN_WGS: developer knob, fewest 16x16 workgroups for the pipelined shapes
    if (plain && wgs16 >= option_int("VP_X3_MIN_WGS", q.plan_latency ? 160 : 100)) halo = want == 6 ? 6 : 7;
  }
  return halo;
}

// step 3, the map kernels.  forced_nsplit is what the caller forced or, as the rules stand, what step 2 picked (see choose_conv)
// parity mode, small maps of the neck (20x40 / 40x80 pixels, long K): one workgroup = a 32-channel weight slab x a K slice x ALL pixels
// of a 20x40 region (kernels_conv3x3_map.hip, halo tile 11): the 8x16 tiles re-stream the weights once per pixel tile and are bound by
// that traffic.  Any epilogue (it always ends in the finish kernel).  VP_MAP3X3=0 (developer knob, A/B timing): the tiled kernels.
int map_tile(const ConvQuery& q, int ncols, int M, int halo) {
  const bool on = !dev_option_is("VP_MAP3X3", '0');
  // round 4: the context block's 10x20 maps take the kernel's 10x20-region geometry (four waves, two workgroups per CU; VP_CTX3=0: the
  // halo kernel's 8x16 tiles + split-K as before) -- context_layer_4 has 128 input channels, so the channel floor is per geometry
  const int geom = conv3x3_map_geometry(q.H, q.W);
  const bool geom_on = geom == 1 ? q.cin_pad >= 256 : (geom == 2 && q.cin_pad >= 128 && !dev_option_is("VP_CTX3", '0'));
  // round 4: the VP_FP16 engines take the kernel too (X1: steps of 32 channels, the halves in the two planes; VP_F16_MAP=0: the halo kernel's
  // 64-channel tiles + split-K as before)
  const char* envf = dev_option("VP_F16_MAP");
  // measured per layer (profiles/r04_layers_sceneseg_fp16_map_ab.tsv, halo kernel + split-K -> map kernel, us): context_layer_4..6 20.5 / 16.5 / 22.7 ->
  // 18.5 / 14.3 / 19.9, decode_layer_0 (1280 channels on 20x40) 40.4 -> 35.5; decode_layer_1..3 28.2 / 43.7 / 37.1 -> 29.9 / 45.5 / 37.8: the kernel
  // where it wins (the 10x20 geometry, >= 1024 input channels on a single region); VP_F16_MAP=1 everywhere it fits
  const bool f16_rule = (envf && envf[0] == '1') || geom == 2 || (q.cin_pad >= 1024 && M <= 800);
  const bool prec_on = q.split || (!q.fp8_storage && q.cin_pad % 32 == 0 && !(envf && envf[0] == '0') && f16_rule);
  const int map_max_m = option_int("VP_MAP_MAX_M", 3200);   // developer knob: largest map (pixels) the map kernels take
  if (q.tile == 111 || (on && prec_on && q.tile < 0 && halo >= 0 && ncols > 32 && !q.logits_out && !q.in2 && M <= map_max_m && geom_on &&
                        conv3x3_map_shape_ok(q.H, q.W, q.cin_pad, round_up(ncols, 32))))
    halo = 11;
  // round 5: 64-channel slabs (two M tiles per wave, kernels_conv3x3_map.hip "map2") where the geometry is the neck's and the output channels pad to 64
  // without waste: parity mode only.  VP_MAP2=0 (developer knob, A/B timing): tile 11 everywhere.
  const int min_regions = option_int("VP_MAP2_MIN_REGIONS", 1);   // developer knob: 4 = the 40x80 maps only
  if (halo == 11 && q.tile < 0 && q.split && geom == 1 && !dev_option_is("VP_MAP2", '0') && !(q.plan_latency && !dev_option_is("VP_MAP2", '1')) &&
      round_up(ncols, 64) == round_up(ncols, 32) &&
      (q.H / 20) * (q.W / 40) >= min_regions && conv3x3_map2_shape_ok(q.H, q.W, q.cin_pad, round_up(ncols, 64)))
    halo = 12;
  if (q.tile == 112) halo = 12;
  return halo;
}

// step 6, the split factor (and K block) for the chosen tile; forced: the caller's factor (<= 0 = the rule's)
void halo_split(const ConvQuery& q, int M, int halo, int forced, ConvChoice* c) {
  const double slice_mb = (double)M * c->CoutW * 4.0 / 1e6;
  if (halo == 12) {  // 64-channel slabs: a workgroup is twice the work of tile 11's, so the SAME K split gives half the workgroups (see the kernel's header)
    const int regions = (q.H / 20) * (q.W / 40), n_co = c->CoutW / 64, KS = q.cin_pad / 16;
    const int slots = std::max(1, option_int("VP_MAP2_SLOTS", 128));   // developer knob: workgroups a layer aims at
    int ns = forced > 0 ? forced : std::max(1, slots / (regions * n_co));
    double cap_mb = 27.0;   // 40x80 maps: four K slices (26.2 MB of slabs) -- measured 124 -> 103 / 91 -> 76 us per layer and +1.1 % frames/s against three (gpurun r5c04)
    if (const char* e = dev_option("VP_MAP2_CAP_MB")) cap_mb = std::atof(e);   // developer knob: ceiling of the fp32 slabs a layer may write
    while (forced <= 0 && ns > 2 && ns * slice_mb > cap_mb) --ns;
    c->bk = 16;
    c->nsplit = std::max(1, std::min(ns, std::max(1, KS / 2)));
    return;
  }
  if (halo == 11) {  // map kernel: K slices until ~one round of workgroups (one per CU at 20x40 regions, two at 10x20), fp32 slabs <= 24 MB
    const int geom = conv3x3_map_geometry(q.H, q.W);
    const int regions = geom == 1 ? (q.H / 20) * (q.W / 40) : (q.H / 10) * (q.W / 20), n_co = c->CoutW / 32, KS = q.cin_pad / (q.split ? 16 : 32);
    const int slots = geom == 1 ? 256 : 512;   // 155 KB of LDS = one workgroup per CU (a 257th waits a whole round); 74 KB = two
    int ns = forced > 0 ? forced : std::max(1, slots / (regions * n_co));
    while (forced <= 0 && ns > 2 && ns * slice_mb > 26.0) --ns;
    if (const char* e = dev_option("VP_MAP_NSPLIT_PCT")) {   // developer knob (K-slice sweeps of the map kernel): percentage of the rule's factor
      if (forced <= 0 && ns > 1) ns = std::max(1, (int)(ns * std::atoi(e) / 100.0 + 0.5));
    }
    c->bk = q.split ? 16 : 32;
    c->nsplit = std::max(1, std::min(ns, std::max(1, KS / 2)));
    return;
  }
  const int KC = q.cin_pad / 32;
  const long long blocks = cdiv(q.H, halo_tile_th(halo)) * cdiv(q.W, 16) * (c->CoutW / halo_tile_co(halo));
  // split-K: aim at ONE machine-wide wave of workgroups (256); go towards two only while the K loop per slice stays
  // long (> 6 chunks = 54 tap steps), and keep the fp32 partials (written + re-read by the finish kernel at
  // ~4.5 TB/s) under ~24 MB.  Measured per layer in profiles/r01_splitk_ablation.txt.
  int ns = 1;
  if (forced > 0) {
    ns = forced;
  } else if (halo == 4 && q.logits_out && q.cout <= 4 && (q.cin_pad == 64 || q.cin_pad == 128) && q.res_mode == RES_NONE && q.act == ACT_NONE &&
             std::max(1, q.stride) == 1 && !(dev_option_is("VP_HEAD_CONV", '0'))) {
    ns = 1;  // a head's logits convolution goes to kernels_head.hip (persistent workgroups: needs no split on any map size)
  } else if (blocks < 256 && q.split) {
    // parity mode (measured per layer with VP_NSPLIT_FORCE = 1..16, profiles/r02_splitk_sweep_fp16x3.txt): ONE full round of
    // workgroups at two per CU -- ns = floor(512 / blocks), at most one slice per input chunk.  A little past 512 (the fp16
    // rule gave 540 / 600 workgroups on the 20x40 / 40x80 layers) a second, nearly empty round costs 10-20 % of the layer.
    ns = (int)std::max<long long>(1, 512 / blocks);
    while (ns > 2 && ns * slice_mb > 24.0) --ns;
  } else if (blocks < 256) {
    ns = (int)((256 + blocks - 1) / blocks);
    while (KC / ns > 6 && blocks * ns < 512) ++ns;
    while (ns > 2 && ns * slice_mb > 24.0) --ns;
    ns = std::min(ns, std::max(1, KC / 2));
  }
  if (const char* e = dev_option("VP_NSPLIT_PCT")) {  // developer knob (split-K sweeps): percentage applied to the heuristic's factor
    if (forced <= 0 && ns > 1) ns = std::max(1, (int)(ns * std::atoi(e) / 100.0 + 0.5));
  }
  if (const char* e = dev_option("VP_NSPLIT_FORCE")) {  // developer knob: one factor for every layer the heuristic splits
    if (forced <= 0 && ns > 1) ns = std::max(1, std::atoi(e));
  }
  c->nsplit = std::max(1, std::min(ns, KC));
  if (halo == 6) c->nsplit = 1;  // one 8-wave workgroup per CU, >= 160 tiles: no split-K shape
}

// step 7, the late moves onto the pipelined 64-channel shapes (halo tiles 8 / 9), which look at the split factor step 6 chose
// 64-channel tiles of the parity mode: the pipelined kernel's 64-channel shape (halo tile 8: same tiles, same split factor as
// halo tile 3, three workgroups per CU).  Measured on MI355X (SceneSeg, us, halo tile 3 -> tile 8): decode_layer_0..3 70.5 /
// 48.1 / 82.6 / 60.2 -> 77.9 / 54.6 / 90.2 / 65.6, decode_layer_5 98.6 -> 106.5, decode_layer_9 (128 -> 64 channels on
// 320x640) 108.0 -> 102.2; 389 -> 381 frames/s with it everywhere.  So: only the short-K big-map case (as for tile 7);
// VP_X3_C64=1 wherever the epilogue fits (plain, or anything behind split-K), =0 nowhere.
int late_c64_tile(const ConvQuery& q, int ncols, int M, int halo, ConvChoice* c) {
  const bool stride1 = std::max(1, q.stride) == 1, plain = plain_epilogue(q);
  if ((halo == 3 || halo == 2) && !q.split && !q.fp8_storage && q.tile < 0 && q.cin_pad % 64 == 0 && ncols == 64 && !q.logits_out && !q.in2 && stride1) {
    // fp16 engines, 64-channel outputs on the big maps (decode_layer_9: 128 -> 64 channels on 320x640): the pipelined 64-channel shape
    const char* e8 = dev_option("VP_F16_BIG");
    if (plain && e8 && e8[0] != '0' && M >= 65536) {   // measured level with the halo kernel (decode_layer_9: 52.2 -> 52.0 us): only when forced
      halo = 8;
      c->nsplit = 1;
    }
  }
  if (halo == 3 && q.split && q.tile < 0 && q.cin_pad % 32 == 0 && !q.logits_out && !q.in2 && stride1) {
    const char* e8 = dev_option("VP_X3_C64");
    const bool fits = plain || c->nsplit > 1;
    const bool want8 = e8 ? e8[0] == '1' : (c->nsplit == 1 && q.cin_pad <= 128 && M >= 65536);
    if (fits && want8) halo = 8;
  }
  // round 5: 64-channel tiles of the parity mode on 16x16 pixels with the four waves side by side (halo tile 9: every wave 64 channels x 64 pixels, 8
  // fragment reads per 12 MFMAs instead of 6 per 6).  Built for the 64-channel-output layers without split-K on VERDICT round 4's reading that they are
  // fragment-read-bound; MEASURED SLOWER (profiles/r05_x3_t16_ab.txt): decode_layer_5 99.2 -> 135.1 us (200 workgroups of four waves = one wave per
  // SIMD on 200 CUs), decode_layer_9 103.9 -> 110.6 us (800 tiles on 512 slots: two rounds), frames/s level (412.8 against 412.7).  Kept as a shape
  // (tile 109, tests), selected only by VP_X3_T16=1.
  if ((halo == 3 || halo == 8) && q.split && q.tile < 0 && c->nsplit == 1 && q.cin_pad % 32 == 0 && !q.logits_out && !q.in2 && stride1 && plain &&
      dev_option_is("VP_X3_T16", '1') && M >= 12800)
    halo = 9;
  return halo;
}

// step 5b, VP_MFMA_FP8: what the e4m3 MFMA kernel (halo tile 13, kernels_conv3x3.hip conv3x3_f8_kernel) can run ...
bool f8_shape_ok(const ConvQuery& q, int ncols) {
  return q.ks == 3 && std::max(1, q.stride) == 1 && !q.split && !q.fp8_storage && !q.in2 && !q.logits_out && plain_epilogue(q) && q.cin_pad >= 64 &&
         q.cin_pad % 64 == 0 && round_up(ncols, 64) == ncols;
}
// ... and which of those layers a flagged engine hands to it: maps of 80 x 160 pixels and larger (below, the fp16 engines' layers are split-K or
// map-kernel layers the kernel has no form for) with at least 512 input channels -- decode_layer_5 of the scene decoders (512 -> 256 on 80 x 160).
// The channel floor is MEASURED (profiles/f8_mfma.txt, us, fp16 kernel -> conv3x3_f8): decode_layer_5 55.4 -> 51.8, but decode_layer_7 (256 -> 128 on
// 160 x 320) 38.2 -> 56.3 and decode_layer_9 (128 -> 64 on 320 x 640) 50.1 -> 60.4: the kernel runs at 500 - 580 TFLOP/s on all three (it quantises its
// halo in VALU instructions, per output-channel tile), the fp16 kernels at 545 / 790 / 600.  VP_PLAN_OVERRIDE "<layer>=13" still puts any layer that
// f8_shape_ok accepts on the kernel (tools/bench_f8.py measures the two excluded layers that way).
bool f8_rule(const ConvQuery& q, int ncols) { return f8_shape_ok(q, ncols) && q.H * q.W >= 12800 && q.cin_pad >= 512; }

}  // namespace

ConvChoice choose_conv(const std::string& name, const ConvQuery& q) {
  const int cstride = std::max(1, q.stride);
  if (cstride > 1 && (q.ks != 3 || q.H % cstride || q.W % cstride)) throw std::invalid_argument("strided conv: 3x3 on even maps only: " + name);
  const int M = (q.H / cstride) * (q.W / cstride), ncols = round_up(q.cout, 32);
  int halo = -1, rule_nsplit = 0;
  if (q.ks == 3 && cstride == 1 && q.H >= 8 && q.W >= 16) {
    halo = base_halo_tile(q, ncols);
    halo = pipelined_tile(q, ncols, halo, &rule_nsplit);
    halo = map_tile(q, ncols, M, halo);
    // steps 4 and 5, the fp8 clamp and the shape validity throws (in the order the messages have always come in)
    if (halo == 12 && (!q.split || q.fp8_storage || !conv3x3_map2_shape_ok(q.H, q.W, q.cin_pad, round_up(ncols, 64))))
      throw std::invalid_argument("halo tile 12 (map kernel, 64-channel slabs): parity mode, maps that tile into 20x40 regions, >= 32 input channels: " + name);
    // VP_WEIGHTS_FP8 as storage (AutoDrive engines and the operator entry): the halo kernel's 8x16-pixel tiles of 64 / 32 channels are the ones
    // instantiated with the byte-weight staging path (kernels_conv3x3.hip W8)
    if (q.fp8_storage && q.tile < 0 && halo >= 0) halo = ncols <= 32 ? 4 : 3;
    if (halo == 11 && (q.fp8_storage || (!q.split && q.cin_pad % 32 != 0) || !conv3x3_map_shape_ok(q.H, q.W, q.cin_pad, round_up(ncols, 32))))
      throw std::invalid_argument("halo tile 11 (map kernel): maps that tile into 20x40 or 10x20 regions, >= 32 input channels (a multiple of 32 in the fp16 engines): " + name);
    if (halo >= 6 && halo <= 9 && !q.split && q.cin_pad % 64 != 0) throw std::invalid_argument("halo tiles 6 - 9 in the fp16 engines: input channels a multiple of 64: " + name);
    // step 5b, VP_MFMA_FP8 (only with the flag): the plain big layers move to the e4m3 MFMA kernel, whatever fp16 kernel the steps above gave them
    if (q.mfma_fp8 && q.tile < 0 && q.nsplit <= 0 && f8_rule(q, ncols)) halo = 13;
    if (halo == 13 && !(q.mfma_fp8 && f8_shape_ok(q, ncols)))
      throw std::invalid_argument("halo tile 13 (e4m3 MFMA kernel): VP_FP16 | VP_MFMA_FP8, 3x3 stride 1, conv + bias + {GELU, none}, input channels a multiple of 64, output channels that pad to a multiple of 64 without waste: " + name);
  }
  ConvChoice c;
  if (halo == 13) {   // one tile shape, no split-K
    c.tile = 113;
    c.bk = 64;
    c.CoutW = round_up(ncols, 64);
    c.nsplit = 1;
    c.layout = F8_K64;
    c.w8 = true;
    return c;
  }
  if (halo >= 0) {
    // The fp16 rule of step 2 picks four K slices WITH halo tile 7, and a later step may still replace the tile: the factor then reaches the new tile's
    // kernel as if the caller had forced it (SceneNeck.decode_layer_0 of the three-op fp16 plan runs the map kernel on 4 slices instead of its own ~10:
    // ADVICE.md, round 6).  Reproduced as it is -- tests/golden/plan_options.json pins it; applying rule_nsplit only while the tile is still 7 is a
    // behaviour change of its own.
    const int forced = q.nsplit > 0 ? q.nsplit : rule_nsplit;
    c.bk = 32;
    c.CoutW = round_up(ncols, halo_tile_co(halo));
    halo_split(q, M, halo, forced, &c);
    if (halo < 11) halo = late_c64_tile(q, ncols, M, halo, &c);
    c.tile = 100 + halo;
    c.layout = halo == 12 ? MAP2 : halo == 11 ? (q.split ? MAP : MAP_K32) : (halo >= 6 && halo <= 9) ? (q.split ? X3_SWIZZLED : X1_K64) : HALO32;
  } else {
    // fp8 storage: the generic kernel's 64 x 64 tile carries the byte-weight staging path (kernels_conv.hip W8)
    c = choose_gemm_cfg(M, ncols, q.cin_pad, q.ks, (q.fp8_storage && q.tile < 0) ? 2 : q.tile, q.bk, q.nsplit);
    c.layout = GEMM_ROWS;   // the LDS-DMA layout is add_convT*'s alone
  }
  // VP_WEIGHTS_FP8: real e4m3 storage where the layer's kernel stages its weights through registers (the generic GEMM kernel and the halo
  // kernel's tiles 0-5: every matrix layer of AutoDrive); the LDS-DMA / register-stationary kernels copy weight images verbatim and keep
  // de-quantised fp16 planes
  c.w8 = q.fp8_storage && ((halo < 0 && c.tile == 2) || halo == 3 || halo == 4);
  return c;
}

// The small-map up-sampling GEMMs go to the LDS-DMA pipelined kernel (kernels_gemm_dma.hip; tile 6).  Measured per layer on
// MI355X (SceneSeg neck, us, old -> new): parity mode 42.1 / 41.0 / 42.2 -> 37.9 / 37.7 / 37.7 and +2.8 % frames/s with three
// frames in flight (fewer workgroups at a higher rate leave CUs to the other frames); fp16 30.4 / 23.4 / 25.4 -> 26.8 / 26.8 /
// 21.7: the fp16 engines take it from 2048 pixels up only.  VP_GEMM_DMA=1: wherever the shape fits, =0: never.
bool gemm_dma_wanted(int H, int W, int ncols, int cin_pad, int cin2_pad, int cstore, bool split) {
  const int M = H * W;
  const char* e = dev_option("VP_GEMM_DMA");
  if (e && e[0] == '0') return false;
  if (!split && M < 2048 && !(e && e[0] == '1')) return false;
  // the register-stationary kernel's shapes are its own (and keep the plain weight layout)
  if (!dev_option_is("VP_CONVT_RS", '0') && convt_rs_shape_case(H, W, cin_pad, cin2_pad, ncols, cstore) != 0) return false;
  return gemm_dma_shape_ok(M, ncols, cin_pad, cin2_pad, cstore);
}

// split-K factor of that kernel: towards ~160 workgroups while a slice keeps >= 8 K steps (VP_GEMM_DMA_NSPLIT: developer knob)
int gemm_dma_nsplit(int M, int ncols, int kw) {
  if (const char* e = dev_option("VP_GEMM_DMA_NSPLIT")) return std::max(1, std::atoi(e));
  const int tiles = ((M + 127) / 128) * (ncols / 256), steps = kw / 32;
  int ns = 1;
  while (tiles * ns < 128 && steps / (ns + 1) >= 8) ++ns;
  return ns;
}

// ------------------------------------------------------------------------------------------- weight packing
size_t pack_index(WeightLayout layout, int co, int ci, int tap, int cin_pad, int CoutW) {
  // the pipelined kernels copy weight tiles to LDS by LDS-DMA, a LINEAR copy: the tile is stored in its LDS image order, i.e. with the 16-byte
  // chunks of a row XOR-swizzled by (row >> 2) & 3
  const int ci_sw = (((ci & 31) >> 3) ^ ((co >> 2) & 3)) << 3 | (ci & 7);
  switch (layout) {
    case GEMM_ROWS: return ((size_t)tap * CoutW + co) * cin_pad + ci;
    case HALO32: return (((size_t)(ci >> 5) * 9 + tap) * CoutW + co) * 32 + (ci & 31);
    case X3_SWIZZLED: return (((size_t)(ci >> 5) * 9 + tap) * CoutW + co) * 32 + ci_sw;
    case X1_K64: return (((size_t)(ci >> 6) * 9 + tap) * CoutW + co) * 32 + ci_sw;
    case MAP: return conv3x3_map_pack_index(co, ci, tap, cin_pad);
    case MAP_K32: return conv3x3_map_pack_index_k32(co, ci, tap, cin_pad);
    case MAP2: return conv3x3_map2_pack_index(co, ci, tap, cin_pad);
    case GEMM_DMA: return gemm_dma_pack_index(co, ci, cin_pad);
    case F8_K64: return (((size_t)(ci >> 6) * 9 + tap) * CoutW + co) * 64 + ((((ci & 63) >> 4) ^ ((co >> 2) & 3)) << 4 | (ci & 15));
  }
  return 0;
}

namespace {

// [rows][K] weights -> {hi, lo | codes, bias, post} of `layout`: per row the power-of-two prescale over its K values (fp8 storage: the row's
// quantisation scale instead -- e4m3 values need no prescale, |q| in [2^-9, 448] are normal fp16 numbers), then every value split into its planes.
// w(r, k): the weight; bias(r): its bias; out_row(r): the row's place in the packed matrix (< rows_alloc); at(out_row, k) -> {index, plane} there.
template <class W, class B, class R, class At>
HostWeights pack_weight_rows(int rows, int K, int rows_alloc, size_t elems, WeightLayout layout, bool split, bool w8, int keep_bits, W&& w, B&& bias,
                             R&& out_row, At&& at) {
  const bool halves = layout == X1_K64 || layout == MAP_K32;   // one fp16 value per weight, spread over the two plane arrays
  HostWeights hw;
  hw.hi.assign(w8 ? 0 : elems / (halves ? 2 : 1), (half_t)0.0f);
  hw.lo.assign(((split || halves) && !w8) ? hw.hi.size() : 0, (half_t)0.0f);
  hw.codes.assign(w8 ? elems : 0, (uint8_t)0);
  hw.bias.assign(rows_alloc, 0.0f);
  hw.post.assign(rows_alloc, 1.0f);
  parallel_rows(rows, [&](int r_begin, int r_end) {
    for (int r = r_begin; r < r_end; ++r) {
      const int n = out_row(r);
      hw.bias[n] = bias(r);
      float amax = 0.0f;
      for (int k = 0; k < K; ++k) {
        const float a = std::fabs(w(r, k));
        if (a > amax) amax = a;   // NaN compares false: split_half reports it
      }
      const int sexp = prescale_exp(amax);
      const float pre = w8 ? 1.0f : std::ldexp(1.0f, sexp);
      hw.post[n] = w8 ? fp8_row_scale(amax) : std::ldexp(1.0f, -sexp);
      for (int k = 0; k < K; ++k) {
        const float v = w(r, k);
        const std::pair<size_t, int> d = at(n, k);
        if (w8) {
          if (!(std::fabs(v) <= 65504.0f)) throw RangeError("weight " + std::to_string(v) + " is outside the fp16 range the matrix pipe carries (|w| <= 65504): re-scale the checkpoint");
          hw.codes[d.first] = e4m3_encode(v / hw.post[n]);   // v / S is on the e4m3 grid up to the fold's float rounding: the nearest code IS the quantiser's
          continue;
        }
        half_t h, l;
        split_half(v, pre, &h, &l, keep_bits);
        (d.second ? hw.lo : hw.hi)[d.first] = h;
        if (split && !halves) hw.lo[d.first] = l;
      }
    }
  });
  return hw;
}

}  // namespace

Engine::PackedConv::PackedConv(const ConvChoice& c) : CoutW(c.CoutW), tile(c.tile), bk(c.bk), nsplit(c.nsplit) {}

void Engine::upload_packed(PackedConv* pc, const HostWeights& hw) {
  if (!hw.codes.empty()) {
    pc->w8 = dupload(hw.codes);
    wbytes_[0] += hw.codes.size();
  } else {
    pc->w_hi = dupload(hw.hi);
    pc->w_lo = hw.lo.empty() ? nullptr : dupload(hw.lo);
    wbytes_[1] += 2 * (hw.hi.size() + hw.lo.size());
  }
  pc->bias = dupload(hw.bias);
  pc->wscale = dupload(hw.post);
}

// ------------------------------------------------------------------------------------------- emission
namespace {

enum ConvKernel { K_MAP, K_MAP2, K_X3, K_HEAD, K_HALO, K_GEMM_DMA, K_CONVT_RS, K_GEMM };

// the kernel instantiation tag of a launch; v = the halo tile (K_X3, K_HALO) or the generic tile (K_GEMM)
std::string conv_kernel_tag(ConvKernel k, const ConvGemmParams& p, int v, int bk, bool sp, bool fuse_decode) {
  const char* splitk = p.nsplit > 1 ? "+splitk" : "";
  const char* decode = fuse_decode ? "+decode" : "";
  switch (k) {
    case K_MAP: return std::string("conv3x3_map<co32,") + (conv3x3_map_geometry(p.H, p.W) == 1 ? "px800," : "px200,") + (sp ? "x3>" : "x1,k32>") + "+splitk";
    case K_MAP2: return "conv3x3_map2<co64,px800,x3>+splitk";
    case K_X3:
      // fp16 engines ("x1"): the same schedule on 64-channel chunks, the chunk's two halves in the two LDS planes (kernels_conv3x3_x3.hip X1)
      return std::string(sp ? "conv3x3_x3" : "conv3x3_x1") + (v == 6 ? "w8<co128,px256" : (v == 7 ? "w4<co128,px128" : (v == 8 ? "w4<co64,px128" : "w4<co64,px256"))) + (sp ? ">" : ",k64>") + splitk;
    case K_HEAD: return std::string("head_conv3x3<c") + std::to_string(p.Cin) + (sp ? ",x3>" : ",x1>") + decode;
    case K_HALO: {
      // ",regepi": the register-GELU single-pass epilogue instantiation (same condition as launch_halo_cfg)
      const bool regepi = !sp && p.act == ACT_GELU_F16 && p.res_mode == RES_NONE && p.store_mode == STORE_NHWC && p.nsplit == 1 && !p.w8;
      return "conv3x3_halo<co" + std::to_string(halo_tile_co(v)) + ",px" + std::to_string(halo_tile_px(v)) + (sp ? ",x3" : ",x1") + (p.w8 ? ",w8" : "") +
             (regepi ? ",regepi>" : ">") + splitk + decode;
    }
    case K_GEMM_DMA: return std::string("gemm_dma<co256,px128,") + (sp ? "x3>" : "x1>") + splitk;
    case K_CONVT_RS: return "convt_rs<k" + std::to_string(p.Cin + p.Cin2) + (sp ? ",x3>" : ",x1>");
    case K_GEMM: {
      const int epi = (p.ks == 1 && !sp && !p.w8) ? regepi_case(p, conv_tile_co(v), sp) : 0;  // same rule as launch_cfg (kernels_conv.hip)
      return "conv_gemm<bk" + std::to_string(bk) + ",co" + std::to_string(conv_tile_co(v)) + ",px" + std::to_string(conv_tile_px(v)) + (sp ? ",x3" : ",x1") +
             (p.w8 ? ",w8" : "") + (epi ? ",regepi" + std::to_string(epi) + ">" : ">") + splitk + decode;
    }
  }
  return std::string();
}

// ---- optional per-layer tile autotune (VP_AUTOTUNE=1 enables; measured +-1 % on the frames-in-flight bench, so
// the static heuristic is the default): time the tile shapes that share this weight packing and keep the fastest.  The K order per output is identical for every tile, so the choice never changes a result bit.
int autotune_halo_tile(const ConvGemmParams& p, int ht, bool sp, hipStream_t stream) {
  std::vector<int> cand;
  for (int c : {0, 1, 2, 3, 4}) {
    if (sp && (c == 0 || c == 2)) continue;
    if (p.CoutW % halo_tile_co(c) != 0) continue;
    if (halo_tile_co(c) > p.CoutW) continue;
    if (p.Ncols <= 32 && c != 4) continue;
    if (p.Ncols > 32 && c == 4) continue;
    cand.push_back(c);
  }
  // Cost = wall time of 6 launches spread over 3 streams: the engine is meant to run with several frames in
  // flight, so what counts is the CU-time a tile shape consumes under contention, not its latency alone.
  hipStream_t ts[3] = {stream, nullptr, nullptr};
  VP_HIP_CHECK(hipStreamCreateWithFlags(&ts[1], hipStreamNonBlocking));
  VP_HIP_CHECK(hipStreamCreateWithFlags(&ts[2], hipStreamNonBlocking));
  double best = 1e30;
  int best_c = ht;
  for (int c : cand) {
    hipError_t e = launch_conv3x3_halo(p, c, sp, stream);  // warm-up (also sets the LDS attribute)
    if (e != hipSuccess) continue;
    VP_HIP_CHECK(hipStreamSynchronize(stream));
    const auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < 6 && e == hipSuccess; ++r) e = launch_conv3x3_halo(p, c, sp, ts[r % 3]);
    for (hipStream_t s : ts) VP_HIP_CHECK(hipStreamSynchronize(s));
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (e == hipSuccess && us < best) {
      best = us;
      best_c = c;
    }
  }
  hipStreamDestroy(ts[1]);
  hipStreamDestroy(ts[2]);
  return best_c;
}

}  // namespace

void Engine::push_conv_op(const std::string& name, const Act* in, const PackedConv& pc, int ks, int ncols, const ConvOpts& o, Act* out,
                          int store_mode, int cout_real) {
  ConvGemmParams p{};
  const int cstride = std::max(1, o.stride);
  // the epilogues read the residual at the element offset they store at (conv_epilogue.hpp: res_hi + o, out_hi + o): one row pitch, one map size
  if (o.res_mode != RES_NONE && o.res && out && (o.res->C != out->C || o.res->H != out->H || o.res->W != out->W))
    throw std::invalid_argument("conv residual: the residual needs the destination's row pitch and map size (" + std::to_string(o.res->C) + " x " +
                                std::to_string(o.res->H) + " x " + std::to_string(o.res->W) + " against " + std::to_string(out->C) + " x " + std::to_string(out->H) +
                                " x " + std::to_string(out->W) + "): " + name);
  p.in_hi = in->hi;
  p.in_lo = in->lo;
  p.H = in->H / cstride;  // output size (== input size for stride 1)
  p.W = in->W / cstride;
  p.stride = cstride;
  p.Hin = in->H;
  p.Win = in->W;
  p.post_act = o.post_act;
  p.Cin = in->C;
  p.w_hi = pc.w_hi;
  p.w_lo = pc.w_lo;
  p.bias = pc.bias;
  p.wscale = pc.wscale;
  p.w8 = pc.w8;
  p.ks = ks;
  p.Ncols = ncols;
  p.CoutW = pc.CoutW;
  p.act = (o.act >= ACT_GELU && o.act <= ACT_SIGMOID && !split()) ? (o.act | ACT_F16) : o.act;  // VP_FP16: reduced-instruction activations (common.hpp)
  p.res_mode = o.res_mode;
  p.res_hi = o.res ? o.res->hi : nullptr;
  p.res_lo = o.res ? o.res->lo : nullptr;
  p.store_mode = store_mode;
  p.out_hi = out ? out->hi : nullptr;
  p.out_lo = out ? out->lo : nullptr;
  p.Cstore = out ? out->C : 0;
  p.out_f32 = o.logits_out;
  p.Creal = cout_real;
  p.zeros = static_cast<const half_t*>(zero_page());
  // the head's logits convolution decodes the mask in its epilogue (one launch and a 2.4 MB re-read less per network)
  const bool fuse_decode = store_mode == STORE_NCHW_F32 && o.logits_out == d_logits_ && d_mask_ && cout_real <= 8 && ncols <= 32 && kind_ >= 0 &&
                           kind_ != 4 && !(dev_option_is("VP_FUSE_DECODE", '0'));
  if (fuse_decode) {
    p.mask_out = d_mask_;
    decode_fused_ = true;
  }
  p.nsplit = pc.nsplit;
  if (o.in2) {
    p.Cin2 = o.in2->C;
    p.in2_delta_hi = o.in2->hi - in->hi;
    p.in2_delta_lo = (in->lo && o.in2->lo) ? o.in2->lo - in->lo : 0;
  }
  const int M = p.H * p.W;
  p.partial = (pc.nsplit > 1 || pc.tile == 111 || pc.tile == 112) ? static_cast<float*>(dalloc((size_t)pc.nsplit * M * pc.CoutW * sizeof(float), false)) : nullptr;
  const int tile = pc.tile, bk = pc.bk;
  const bool sp = split();
  Op op;
  op.name = name;
  // VP_ACT_SCALE: the launch reads its tensors' exponents when it RUNS (vp_calibrate_range / vp_set_act_scales change them and invalidate the graph).  With
  // every exponent 0 the block is the unflagged engine's, bit for bit; otherwise `scaled` sends it to the all-runtime epilogue (conv_epilogue.hpp).
  const Act* res_act = o.res;
  auto with_exps = [this, in, res_act, out](ConvGemmParams q) {
    const int si = act_exp(in), sr = act_exp(res_act), so = act_exp(out);
    q.scaled = (si | sr | so) != 0;
    q.in_mul = std::ldexp(1.0f, si);
    q.res_mul = std::ldexp(1.0f, sr);
    q.out_mul = std::ldexp(1.0f, -so);
    return q;
  };
  // a launch with the patches it takes when it RUNS: the decode mode of a fused decode (vp_set_decode_mode may change it between frames; it
  // invalidates the graph), the exponents of a VP_ACT_SCALE engine; an unflagged engine passes its parameter block untouched
  auto patched = [&](auto launch) -> std::function<hipError_t(hipStream_t)> {
    if (fuse_decode)
      return [this, p, launch](hipStream_t st) {
        ConvGemmParams q = p;
        q.decode_mode = decode_mode_;
        return launch(q, st);
      };
    if (act_scale()) return [p, launch, with_exps](hipStream_t st) { return launch(with_exps(p), st); };
    return [p, launch](hipStream_t st) { return launch(p, st); };
  };
  if (act_scale()) {
    const bool halo_plain = tile >= 100 && tile - 100 <= 5 && !(tile == 104 && o.tile < 0 && head_conv_supported(p));
    if (!(halo_plain || tile < 5) || store_mode != STORE_NHWC || o.in2 || fuse_decode || !out || (o.tile < 0 && tile < 100 && convt_rs_supported(p, sp)))
      throw std::invalid_argument("VP_ACT_SCALE: only the generic GEMM kernel and the halo kernel's tiles 0 - 5 (NHWC store) carry the activation scale: " + name);
  }
  if (out) op.writes = {out};
  if (pc.nsplit > 1) op.launch = "nsplit=" + std::to_string(pc.nsplit);   // the tag only says "+splitk"
  op.flops = 2.0 * M * (double)cout_real * (store_mode == STORE_SHUFFLE2 ? 4 : 1) * in->Creal * ks * ks;
  const double esz = sp ? 4.0 : 2.0;
  op.bytes = esz * ((double)M * in->Creal + (double)M * (store_mode == STORE_SHUFFLE2 ? 4 : 1) * cout_real) +
             (pc.w8 ? 1.0 : esz) * ((double)cout_real * (store_mode == STORE_SHUFFLE2 ? 4 : 1) * in->Creal * ks * ks);
  if (o.in2) {  // fused skip-link: extra K columns read at every OUTPUT pixel
    op.flops += 2.0 * M * 4.0 * cout_real * o.in2->Creal;
    op.bytes += esz * ((double)M * 4.0 * o.in2->Creal + (double)cout_real * o.in2->Creal);
  }
  int ht = tile - 100;
  if (tile >= 100 && ht != 13 && o.tile < 100 && dev_option_is("VP_AUTOTUNE", '1') && kind_ >= 0) ht = autotune_halo_tile(p, ht, sp, stream_);
  // the heads' logits convolution: weights stationary in registers, 16x16x32 MFMA, LDS-DMA halo (kernels_head.hip); same weight
  // packing as halo tile 4.  VP_HEAD_CONV=0 keeps the halo kernel.
  const bool head = tile >= 100 && ht == 4 && o.tile < 0 && head_conv_supported(p) && !(dev_option_is("VP_HEAD_CONV", '0'));
  if (tile >= 100 && ht == 13) {
    // VP_MFMA_FP8: the launch reads its layer's qexp when it RUNS (vp_calibrate_fp8 / vp_set_fp8_exps change it and invalidate the graph)
    p.f8_qmul = p.f8_smul = 1.0f;
    if (!mfma_fp8() || !conv3x3_f8_supported(p))
      throw std::invalid_argument("halo tile 13 (e4m3 MFMA kernel): VP_FP16 | VP_MFMA_FP8, conv + bias + {GELU, none}, NHWC, input and output channels multiples of 64: " + name);
    Fp8Layer fl;
    fl.op = ops_.size();
    for (size_t t = 0; t < acts_.size(); ++t)
      if (acts_[t].get() == in) fl.tensor = (int)t;
    const size_t slot = f8_layers_.size();
    f8_layers_.push_back(fl);
    op.kernel = "conv3x3_f8";
    op.run = [this, p, slot](hipStream_t st) {
      ConvGemmParams q = p;
      const int e = f8_layers_[slot].qexp;
      q.f8_qmul = std::ldexp(1.0f, -e);
      q.f8_smul = std::ldexp(1.0f, e);
      return launch_conv3x3_f8(q, st);
    };
  } else if (tile >= 100 && ht == 11) {
    if (!conv3x3_map_supported(p)) throw std::invalid_argument("halo tile 11 (map kernel): 3x3 stride 1, 20x40 or 10x20 regions: " + name);
    op.kernel = conv_kernel_tag(K_MAP, p, ht, bk, sp, fuse_decode);
    op.run = [p](hipStream_t st) { return launch_conv3x3_map(p, st); };
  } else if (tile >= 100 && ht == 12) {
    if (!conv3x3_map2_supported(p)) throw std::invalid_argument("halo tile 12 (map kernel, 64-channel slabs): parity mode, 3x3 stride 1, 20x40 regions, output channels padded to 64: " + name);
    op.kernel = conv_kernel_tag(K_MAP2, p, ht, bk, sp, fuse_decode);
    op.launch += " wgs=" + std::to_string((p.H / 20) * (p.W / 40) * (p.CoutW / 64) * p.nsplit);
    op.run = [p](hipStream_t st) { return launch_conv3x3_map2(p, st); };
  } else if (tile >= 100 && ht >= 6 && ht <= 9) {
    if (!conv3x3_x3_supported(p, ht)) throw std::invalid_argument("halo tiles 6 - 9 (pipelined kernels): conv + bias + {GELU, none}, NHWC, 128- (64-) channel tiles, fp16: input channels a multiple of 64; any epilogue with split-K (7 / 8): " + name);
    op.kernel = conv_kernel_tag(K_X3, p, ht, bk, sp, fuse_decode);
    op.run = [p, ht](hipStream_t st) { return launch_conv3x3_x3(p, ht, st); };
  } else if (head) {
    const void* zeros = zero_page();
    op.kernel = conv_kernel_tag(K_HEAD, p, ht, bk, sp, fuse_decode);
    op.run = patched([zeros](const ConvGemmParams& q, hipStream_t st) { return launch_head_conv(q, zeros, st); });
  } else if (tile >= 100) {
    op.kernel = conv_kernel_tag(K_HALO, p, ht, bk, sp, fuse_decode);
    op.run = patched([ht, sp](const ConvGemmParams& q, hipStream_t st) { return launch_conv3x3_halo(q, ht, sp, st); });
  } else if (tile == 6) {  // its weights are packed in its own layout (add_convT*): no other kernel may take this launch
    if (!gemm_dma_supported(p, sp))
      throw std::invalid_argument("LDS-DMA GEMM kernel (tile 6): ConvTranspose k2 s2 (+ skip link) + bias, 4 * Cout and Cout multiples of 256, K >= 256, >= 128 pixels: " + name);
    op.kernel = conv_kernel_tag(K_GEMM_DMA, p, tile, bk, sp, fuse_decode);
    op.run = [p](hipStream_t st) { return launch_gemm_dma(p, st); };
  } else if (tile == 5 || (!(dev_option_is("VP_CONVT_RS", '0')) && convt_rs_supported(p, sp))) {
    if (!convt_rs_supported(p, sp))
      throw std::invalid_argument("register-stationary ConvTranspose kernel (tile 5): k2 s2 + bias, K = 128 or 256 + 32 (skip link), map width a multiple of 32, >= 2048 pixels: " + name);
    op.kernel = conv_kernel_tag(K_CONVT_RS, p, tile, bk, sp, fuse_decode);
    // Round 5: the K = 256 + 32 case (ConvTranspose + skip link 80x160 -> 160x320: four quadrant slices per pixel range) runs on 32 pixel-tile groups per
    // slice = 128 persistent workgroups instead of 256.  An HBM-side byte mover does not need every CU to pull its bytes: ALONE the launch is slower
    // (37.8 -> 52.7 us), with the other head or other cameras on the freed CUs the frame gains 1.2-1.3 % on two boxes and one camera's p50 is level or
    // better (profiles/r05_convt_groups_ab.txt: 403.6 / 402.9 -> 408.4, 414.4 / 413.5 -> 418.7 / 419.9 frames/s; 24 groups +0.7 %, the K = 128 case at
    // 192 / 128 groups +-0).  VP_CONVT_RS_GROUPS_K288 / VP_CONVT_RS_GROUPS (developer knobs, one per shape case) override; both are read HERE, at plan
    // time, and are part of the plan hash.
    if (p.Cin2 > 0 && !plan_latency()) p.rs_groups = 32;
    if (const char* e = dev_option(p.Cin2 > 0 ? "VP_CONVT_RS_GROUPS_K288" : "VP_CONVT_RS_GROUPS")) p.rs_groups = std::max(1, std::atoi(e));
    if (p.rs_groups > 0) op.launch += "groups=" + std::to_string(p.rs_groups);
    op.run = [p](hipStream_t st) { return launch_convt_rs(p, st); };
  } else {
    op.kernel = conv_kernel_tag(K_GEMM, p, tile, bk, sp, fuse_decode);
    op.run = patched([tile, bk, sp](const ConvGemmParams& q, hipStream_t st) { return launch_conv_gemm(q, tile, bk, sp, st); });
  }
  ops_.push_back(std::move(op));
}

// w: [cout][cin][ks][ks] fp32 (already BN-folded where applicable), b: [cout]
Act* Engine::add_conv(const std::string& name, const Act* in, const std::vector<float>& w, const std::vector<float>& b, int cout, int ks,
                      const ConvOpts& o_in, Act* out_override) {
  ConvOpts o = o_in;
  {
    int ot = -1, on = 0;   // one layer's choice forced by name (VP_PLAN_OVERRIDE: the in-frame tuner)
    if (ks == 3 && o.tile < 0 && plan_override(name, &ot, &on)) {
      o.tile = 100 + ot;
      if (on > 0) o.nsplit = on;
    }
  }
  const int cin = in->Creal, cin_pad = in->C, taps = ks * ks;
  if (w.size() != (size_t)cout * cin * taps) throw std::runtime_error("conv weight size mismatch: " + name);
  // the kernels take the input's channel count as its row pitch (the comment in front of build_autospeed): an alias view narrower than its tensor is no input
  if (in->C != round_up(in->Creal, 32)) throw std::invalid_argument("conv input: a convolution's input cannot be a slice of a wider tensor: " + name);
  ConvQuery q;
  q.H = in->H, q.W = in->W, q.stride = o.stride;
  q.cin = cin, q.cin_pad = cin_pad, q.cout = cout, q.ks = ks;
  q.act = o.act, q.res_mode = o.res_mode, q.post_act = o.post_act;
  q.logits_out = o.logits_out != nullptr, q.in2 = o.in2 != nullptr;
  q.tile = o.tile, q.bk = o.bk, q.nsplit = o.nsplit;
  q.split = split(), q.fp8_storage = fp8_storage(), q.plan_latency = plan_latency();
  q.mfma_fp8 = mfma_fp8();
  const ConvChoice c = choose_conv(name, q);
  PackedConv pc(c);
  const HostWeights hw = pack_weight_rows(
      cout, cin * taps, c.CoutW, (size_t)taps * c.CoutW * cin_pad, c.layout, split(), c.w8, wlo_keep_,
      [&](int co, int k) { return w[(size_t)co * cin * taps + k]; }, [&](int co) { return b[co]; }, [](int co) { return co; },
      [&](int co, int k) { return std::pair<size_t, int>(pack_index(c.layout, co, k / taps, k % taps, cin_pad, c.CoutW), pack_plane(c.layout, k / taps)); });
  upload_packed(&pc, hw);
  const int cstride = std::max(1, o.stride);
  Act* out = nullptr;
  int store = STORE_NHWC;
  if (o.logits_out) {
    store = STORE_NCHW_F32;
  } else {
    out = out_override ? out_override : new_act(name, cout, in->H / cstride, in->W / cstride);
  }
  push_conv_op(name, in, pc, ks, round_up(cout, 32), o, out, store, cout);
  return out;
}

// ConvTranspose2d(k2,s2) [+ the 1x1 skip link as a K extension, cs >= 0 channels behind cin_pad]: wt [cin][cout][2][2], ws [cout][cs] -> GEMM rows
// n = (dy*2+dx)*cpad + co over input pixels, the prescale per GEMM row over BOTH weight sets of its K axis, the biases summed
static HostWeights pack_convT_rows(const std::vector<float>& wt, const std::vector<float>& bt, const float* ws, const float* bs, int cin, int cin_pad,
                                   int cs, int cs_pad, int cout, int cpad, const ConvChoice& c, bool split, int keep_bits) {
  const int kw = cin_pad + cs_pad;
  auto weight = [&](int r, int k) {  // wt: [ci][co][dy][dx], q = dy*2+dx
    const int q = r / cout, co = r - q * cout;
    return k < cin ? wt[((size_t)k * cout + co) * 4 + q] : ws[(size_t)co * cs + (k - cin)];
  };
  return pack_weight_rows(
      4 * cout, cin + cs, c.CoutW, (size_t)c.CoutW * kw, c.layout, split, false, keep_bits, weight, [&](int r) { return bs ? bt[r % cout] + bs[r % cout] : bt[r % cout]; },
      [&](int r) { return (r / cout) * cpad + r % cout; },
      [&](int n, int k) { return std::pair<size_t, int>(pack_index(c.layout, n, k < cin ? k : cin_pad + (k - cin), 0, kw, c.CoutW), 0); });
}

static const char* const kGemmDmaShape = "LDS-DMA GEMM kernel (tile 6): ConvTranspose k2 s2 (+ skip link) + bias, 4 * Cout and Cout multiples of 256, K >= 256, >= 128 pixels: ";

// ConvTranspose2d(k2,s2): w [cin][cout][2][2] -> GEMM rows n = (dy*2+dx)*Cout_pad + co over input pixels.
Act* Engine::add_convT(const std::string& name, const Act* in, const std::vector<float>& w, const std::vector<float>& b, int cout,
                       const ConvOpts& o) {
  const int cin = in->Creal, cin_pad = in->C;
  if (w.size() != (size_t)cin * cout * 4) throw std::runtime_error("convT weight size mismatch: " + name);
  Act* out = new_act(name, cout, in->H * 2, in->W * 2);
  const int cpad = out->C;
  const int ncols = 4 * cpad;
  ConvOpts oo = o;
  oo.pixel_shuffle = true;
  // parity mode: 128-channel tiles with 32-channel K blocks (measured with VP_CONVT_TILE / VP_CONVT_BK over all tiles:
  // upsample_layer_4 80.9 -> 62.5 us, upsample_layer_1 + skip 54.7 -> 41.6 us, the others unchanged)
  if (split() && oo.tile < 0 && ncols % 128 == 0) {
    oo.tile = 0;
    if (oo.bk < 0) oo.bk = 32;
  }
  if (gemm_dma_wanted(in->H, in->W, ncols, cin_pad, 0, cpad, split()) && o.tile < 0) {
    oo.tile = 6;
    oo.nsplit = gemm_dma_nsplit(in->H * in->W, ncols, cin_pad);
  }
  oo.tile = option_int("VP_CONVT_TILE", oo.tile);  // developer knobs (tile / BK sweeps)
  oo.bk = option_int("VP_CONVT_BK", oo.bk);
  const ConvChoice c = choose_gemm_cfg(in->H * in->W, ncols, cin_pad, 1, oo.tile, oo.bk, oo.nsplit);
  if (c.tile == 6 && !(gemm_dma_shape_ok(in->H * in->W, ncols, cin_pad, 0, cpad) && c.CoutW == ncols))  // before the weights are packed in its layout
    throw std::invalid_argument(kGemmDmaShape + name);
  PackedConv pc(c);
  upload_packed(&pc, pack_convT_rows(w, b, nullptr, nullptr, cin, cin_pad, 0, 0, cout, cpad, c, split(), wlo_keep_));
  push_conv_op(name, in, pc, 1, ncols, o, out, STORE_SHUFFLE2, cout);
  return out;
}

// d = ConvTranspose2d(k2,s2)(x) + Conv1x1(skip) in ONE GEMM (scene_neck.py:29-31 and the other up/skip pairs): the
// skip conv's input channels are appended to the K axis (kernels_conv.hip, K extension), biases are summed.  The
// intermediate up-sampled tensor is never written or re-read (it was the largest HBM stream of these layers) and the
// skip-link launch disappears.  Falls back to the two-op form when a workgroup's channel tile would straddle
// pixel-shuffle quadrants.
Act* Engine::add_convT_skip(const std::string& up_name, const std::string& skip_name, const Act* in, const Act* skip_in,
                            const std::vector<float>& wt, const std::vector<float>& bt, const std::vector<float>& ws,
                            const std::vector<float>& bs, int cout) {
  const int cin = in->Creal, cin_pad = in->C, cs = skip_in->Creal, cs_pad = skip_in->C;
  if (wt.size() != (size_t)cin * cout * 4) throw std::runtime_error("convT weight size mismatch: " + up_name);
  if (ws.size() != (size_t)cout * cs) throw std::runtime_error("skip conv weight size mismatch: " + skip_name);
  if (skip_in->H != in->H * 2 || skip_in->W != in->W * 2) throw std::runtime_error("skip tensor size mismatch: " + skip_name);
  const int cpad = round_up(cout, 32);
  const int ncols = 4 * cpad;
  ConvOpts o;
  o.in2 = skip_in;
  if ((cin_pad | cs_pad) % 64 != 0) o.bk = 32;  // K steps must not straddle the two tensors
  if (split() && ncols % 128 == 0) {  // parity mode: see add_convT
    o.tile = 0;
    o.bk = 32;
  }
  if (gemm_dma_wanted(in->H, in->W, ncols, cin_pad, cs_pad, cpad, split())) {
    o.tile = 6;
    o.nsplit = gemm_dma_nsplit(in->H * in->W, ncols, cin_pad + cs_pad);
  }
  o.tile = option_int("VP_CONVT_TILE", o.tile);
  const ConvChoice c = choose_gemm_cfg(in->H * in->W, ncols, cin_pad + cs_pad, 1, o.tile, o.bk, o.nsplit);
  if (c.tile == 6 && !(gemm_dma_shape_ok(in->H * in->W, ncols, cin_pad, cs_pad, cpad) && c.CoutW == ncols))
    throw std::invalid_argument("LDS-DMA GEMM kernel (tile 6): shape not covered: " + up_name);
  const bool fusable = (cpad % conv_tile_co(c.tile) == 0 && !dev_option_is("VP_FUSE_SKIP", '0')) || c.tile == 6;
  if (!fusable) {
    Act* u = add_convT(up_name, in, wt, bt, cout, ConvOpts{});
    ConvOpts so;
    so.res_mode = RES_ADD;
    so.res = u;
    add_conv(skip_name, skip_in, ws, bs, cout, 1, so, u);
    return u;
  }
  Act* out = new_act(up_name, cout, in->H * 2, in->W * 2);
  PackedConv pc(c);
  upload_packed(&pc, pack_convT_rows(wt, bt, ws.data(), bs.data(), cin, cin_pad, cs, cs_pad, cout, cpad, c, split(), wlo_keep_));
  push_conv_op(up_name + "+" + skip_name.substr(skip_name.rfind('.') == std::string::npos ? 0 : skip_name.rfind('.') + 1), in, pc, 1, ncols, o,
               out, STORE_SHUFFLE2, cout);
  return out;
}

}  // namespace vp

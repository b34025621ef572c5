// zly_internal.h -- shared declarations between the engine (engine.cpp) and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string>
#include "zly.h"
#include "front_variants.h"

namespace zly {

typedef __bf16 bf16_t;

// One frame as the preprocess/decode kernels see it.
struct FrameDesc {
    unsigned long long src_off;   // byte offset of the frame's first pixel in the source buffer; the top byte holds the pixel format (ZLY_PIX_*)
    int w, h;                     // request width / height (REQUEST dims: used for box normalisation too)
};
// The pixel format rides in the top byte of FrameDesc::src_off (the descriptor stays 16 bytes, one load).  A BGR frame's top byte is 0, so the
// BGR-only front-kernel instantiations, which are launched on batches without a YUV frame only, read src_off as the plain offset.
#define ZLY_DESC_FMT_SHIFT 56
__host__ __device__ __forceinline__ unsigned long long desc_pack(unsigned long long off, int fmt) { return off | ((unsigned long long)fmt << ZLY_DESC_FMT_SHIFT); }
__host__ __device__ __forceinline__ unsigned long long desc_off(unsigned long long v) { return v & ((1ull << ZLY_DESC_FMT_SHIFT) - 1); }
__host__ __device__ __forceinline__ int desc_fmt(unsigned long long v) { return (int)(v >> ZLY_DESC_FMT_SHIFT); }

// What a frame view (zly_frame_view, include/zly.h) adds to a frame's descriptor: the offsets of planes 1 and 2 and the three row pitches; plane 0's
// offset is FrameDesc::src_off, the view's size FrameDesc::w, h.  32 bytes = two 16-byte scalar loads, uniform per workgroup.  The n records of a
// call lie right behind its n descriptors (desc + n), so no kernel argument changes; only the VIEW instantiations of the front kernels
// (kernels_view.hip) read them.
struct ViewRec {
    unsigned long long off1, off2;   // byte offset of the region's first sample in plane 1 / plane 2 (unused planes: 0)
    int pitch0, pitch1, pitch2;      // bytes from one row of plane p to the next
    int pad_;
};

// Implicit-GEMM convolution launch arguments.  All tensors are NHWC, batch-major; a tensor
// "view" is a channel slice [co, co+C) of a buffer whose pixels are `cs` elements apart, which is
// how C2f split / Concat cost nothing.
struct ConvArgs {
    // Field ORDER matters on the latency path: kernel arguments are fetched by scalar loads where they are first used, adjacent fields by one wide load, and
    // every further round (s_load ... s_waitcnt) in front of a ~3 us launch's first global load is ~0.1 us, thirty times per batch-1 step (measured: the two
    // reciprocals at the END of this struct cost the step 2.4 %, next to Wo / Ho they gain 1 %).  So: what the index arithmetic and the first loads need
    // comes first, in the order of use; what only the epilogue needs comes last.
    const void* in;               // input tensor (NHWC)
    // 1x1 convs only: fused "nearest-2x Upsample + Concat" input (yolov8.yaml layers 10-11, 13-14).  When in2 is
    // set, input channels [0, split_c) are read from `in`, a tensor of HALF the spatial size, at (y>>1, x>>1),
    // and channels [split_c, Cin) from `in2` at full size.  split_c is a multiple of the k-step.
    const void* in2;
    const void* wgt;              // tiled [CoutPad/16][Kpad/KSTEP][16][KSTEP]
    const float* bias;            // [CoutPad] (requested before the k-loop: with the hot fields)
    int M;                        // batch*Ho*Wo
    int cout_pad;                 // output channels the weight tiles cover (multiple of 16, >= Cout; may include whole zero tiles so that the tile count suits a kernel's channel blocking); read first by the multi-conv kernel's extent test
    int nk;                       // Kpad / KSTEP
    int Ho, Wo;
    float inv_wo, inv_ho;         // 1 / Wo, 1 / Ho: set by launch_conv / launch_conv_multi for the split-K kernel (index arithmetic by reciprocal multiplies)
    int stride, pad;
    int H, W;                     // input spatial size
    int in_cs, in_co;
    int Cin;                      // input channels as stored (multiple of 8)
    int in2_cs, in2_co, split_c;
    int K;                        // ks*ks*Cin
    // ---- epilogue ----
    void* out;        int out_cs, out_co;
    int Cout;
    const void* res;  int res_cs, res_co;    // optional residual (added after the activation)
    int act;                      // 1 = SiLU
    int out_f32;                  // 1 = write fp32 regardless of the activation dtype
};

struct ConvArgsMulti { ConvArgs a[6]; int n; };       // independent convs of one launch (conv_igemm_multi_kernel)
hipError_t launch_conv_multi(const ConvArgsMulti& m, int ct, hipStream_t s);

// Every tuning / test switch of the environment, with its default.  THE list of the switches: an engine reads them once, at zly_create
// (engine.cpp: read_switches), and hands the record to whoever plans a launch; nothing else in csrc/ looks at the environment.
struct Switches {
    int  num_cus = 256;             // compute units the engine's streams may use: the whole chip, or the size of its partition (ZLY_CU_PART).  Persistent grids are
                                    // sized from it (a persistent workgroup that waits for a slot runs a whole round alone)
    // ---- engine ----
    int  cu_part_i = 0, cu_part_n = 1;  // ZLY_CU_PART="i/n": the engine's streams use the i-th of n equal slices of the chip's compute units
    bool no_lanes = false;          // ZLY_NO_LANES (or ZLY_CU_PART given): no Detect branches on side streams
    bool no_c2f = false;            // ZLY_NO_C2F: no fused C2f kernel
    bool no_det_merge = false;      // ZLY_NO_DET_MERGE: the Detect convs as launches of their own at batch <= 4 too
    bool no_tail_split = false;     // ZLY_NO_TAIL_SPLIT: one Detect tail launch for all levels also with side streams
    int  tail_box = 1;              // ZLY_TAIL_BOX: the box branch's second conv (cv2.L.1) inside the Detect tail, at surviving anchors only: 0 = never, 1 = where the tail's early-out is
                                    // live (no head tensor, no logit dump) and conf_thr >= tail_box_min_conf, 2 = wherever the dense launch's k-step order can be reproduced (tests)
    float tail_box_min_conf = 0.05f;    // ZLY_TAIL_BOX_MIN_CONF: lowest confidence threshold at which the automatic mode takes it (the tail's cost per surviving tile is a multiple of the dense kernel's).
                                    // 0.05 is the lowest threshold tried, NOT a measured break-even: from 0.25 down nearly every wave survives and the step is 2-4 ms of NMS, in which
                                    // the tail's growth could not be told from noise (profiles/r06_ab_tail_box.txt; the tail alone per surviving fraction: r06_head_bench_tail_box.txt)
    bool sppf_fused = false;        // ZLY_SPPF_FUSED: the fused SPPF kernel (opt-in: 36 -> ~24 us in isolation at batch 64, but the step gets 0.5 % slower)
    bool pool_six_pass = false;     // ZLY_SPPF_POOL_LDS: SPPF's pools on the six-pass LDS kernel also on small maps
    bool no_wsk = false;            // ZLY_NO_WSK: the class-branch convs on the LDS-tiled kernel (96-channel padding)
    bool nms_general = false;       // ZLY_NMS_GENERAL: every frame on NMS's eight-wave path
    bool no_cout_pad = false;       // ZLY_NO_COUT_PAD: no sixth, all-zero output tile for the 80-channel 3x3 convs
    bool no_cin_pad = false;        // ZLY_NO_CIN_PAD: the class branch's input not stored as a multiple of 32 channels
    bool no_stem1 = false;          // ZLY_NO_STEM1: model.1 not fused into the front kernel
    int  stem1_nw = 0;              // ZLY_STEM1_NW: waves per workgroup of the front kernel (12 / 16; 0 = its default)
    int  stem1_var = 1;             // ZLY_STEM1_VAR: 2 = persistent workgroups + input prefetch, 1 = one tile per workgroup, 0 = round 3's staging / tap order
    int  stem1_grid = 0;            // ZLY_STEM1_GRID: workgroups of the persistent grid (0 = as many as stay resident)
    int  stem1_tw = 0, stem1_th = 0;    // ZLY_STEM1_TW (8..26) / ZLY_STEM1_TH (2..8): the front kernel's tile (0 = planned)
    bool stem1_keep_tiles = false;  // ZLY_STEM1_TW, ZLY_STEM1_TH or ZLY_STEM1_BIG_TILES given: the planned tile at every batch size (no halving for small batches)
    int  pair_min_tiles = 32;       // ZLY_PAIR_MIN_TILES: fewest tiles for which a bottleneck runs as the fused pair
    int  pair_widths = 48;          // ZLY_PAIR_WIDTHS: bit mask of fused pair widths (16 | 32 | 64)
    int  stage_slots = 6;           // ZLY_STAGE_SLOTS: ring slots of the pipelined host path (3..16)
    int  stage_mb = 0;              // ZLY_STAGE_MB: bytes per slot in MiB (0 = 1.25 batches)
    int  inflight = 2;              // ZLY_INFLIGHT: batches on the device at once
    bool d2h_stream = false;        // ZLY_D2H_STREAM: result download on a stream of its own
    int  profile_inner = 1;         // ZLY_PROFILE_INNER: launches per event pair in zly_profile_ops (which reads it per call: bench.py changes it between two calls)
    std::string ablate;             // ZLY_ABLATE_SKIP: ops to leave out, ",name,name," (result-changing: libzly_diag.so only)
    // ---- generic convs (kernels_conv.hip: conv_plan) ----
    bool no_stream = false;         // ZLY_NO_STREAM: never the streaming 1x1 kernel
    bool stream_ct2 = false;        // ZLY_STREAM_CT2: 192 / 256 input channels on its CT = 2 shapes
    int  stream_max_nk = 1 << 30;   // ZLY_STREAM_MAX_NK: most k-steps it takes
    long stream_min_groups = 4096;  // ZLY_STREAM_MIN_GROUPS: fewest pixel groups it takes
    int  stream_wgs = 0;            // ZLY_STREAM_WGS: its persistent workgroups in all (0 = 4, or 2, per CU)
    int  ws1_mode = 1;              // ZLY_WS1: 0 = never the weight-stationary 1x1 kernel, 1 = for the shapes the streaming kernel does not take, 2 = before it
    bool ws1_no_dual = false;       // ZLY_WS1_NO_DUAL: not for the Upsample + Concat inputs
    long ws1_min_px = 2048;         // ZLY_WS1_MIN_PX: fewest pixels it takes
    bool ws1_max_bytes = false;     // ZLY_WS1_MAX_BYTES: plan its shapes as tensors beyond 32-bit offsets are (the direct kernel)
    bool no_ws = false;             // ZLY_NO_WS: never the weight-stationary 3x3 kernel
    bool no_ws_s2 = false;          // ZLY_NO_WS_S2: not for stride 2
    bool no_ws_s2_c32 = false;      // ZLY_NO_WS_S2_C32: not for stride 2 with 32 input channels
    bool ws_rowt = false;           // ZLY_WS_ROWT: its row-tile form (one MFMA tile per output row, kx taps by DPP shifts)
    int  ws_tpw1_maxct = 6;         // ZLY_WS_TPW1_MAXCT: 64 -> 64 as 4 waves x one tile on pixel tiles of up to this many column tiles (0 = never)
    long ws_min_tiles = 64;         // ZLY_WS_MIN_TILES: fewest 13 x 13 tiles' worth of pixels it (and the K-packed kernel) takes
    size_t ws_max_bytes = (size_t)1 << 31;  // ZLY_WS_MAX_BYTES: tensors of this size or more take the LDS-tiled / direct kernel (32-bit offsets; tests lower it)
    int  ws_pair = 1;               // ZLY_WS_PAIR: a 64-channel bottleneck whose two 3x3 convs both plan as the weight-stationary kernel runs as one launch of conv3x3_ws_pair_kernel (0 = the two launches)
    int  ws_pair_max_tiles = 2;     // ZLY_WS_PAIR_MAX_TILES: most tiles per resident workgroup (two per CU) for which it is planned; larger launches keep the two kernels
    int  ws_pair_grid = 0;          // ZLY_WS_PAIR_GRID: most workgroups of its persistent grid (tests: every workgroup walks several tiles; 0 = two per CU)
    bool no_wres = false;           // ZLY_NO_WRES: LDS-tiled kernel without resident weights
    int  wres_maxchunks = 1;        // ZLY_WRES_MAXCHUNKS: most 32-channel chunks whose weights stay resident
    bool lds_s2_pt1 = false;        // ZLY_LDS_S2_PT1: 4-row tiles at stride 2
    long lds_min_tiles = 384;       // ZLY_LDS_MIN_TILES: fewest work items it takes
    int  lds_wgs_per_cu = 0;        // ZLY_LDS_WGS_PER_CU: its persistent workgroups per CU (0 = as many as are resident)
    long direct_pt4_min = 1024, direct_pt2_min = 512;   // ZLY_DIRECT_PT4_MIN / ZLY_DIRECT_PT2_MIN: fewest workgroups for 4 / 2 pixel tiles per wave
    int  direct_ksplit_nk = 1 << 30;    // ZLY_DIRECT_KSPLIT_NK: launches with this many k-steps or more take the 4-way split-K shape whatever their size
    // ---- fused C2f (kernels_pair.hip, kernels_c2f64.hip) ----
    int  c2f32_nw = 0;              // ZLY_C2F32_NW: 8 or 16 waves per workgroup of the 32-channel kernel in every mode (0 = per mode)
    int  c2f_lds_kb = 0;            // ZLY_C2F_LDS_KB: LDS budget of a tile in KiB (0 = 160)
    int  c2f_tile_th = 0, c2f_tile_tw = 0;  // ZLY_C2F_TILE="th,tw": only this tile shape (0 = planned)
    bool c2f64 = false;             // ZLY_C2F64: the fused 64-channel C2f kernel (opt-in: faster per launch, slower per step with three engines)
};

// kernels_conv.hip
// A conv launch, resolved: which kernel, its shape parameters, geometry, grid and dynamic LDS.  conv_plan decides everything (also that a tensor
// beyond a kernel's 32-bit offsets takes another kernel); launch_conv only launches.
enum ConvKind { CONV_DIRECT, CONV_LDS, CONV_STREAM, CONV_WS, CONV_WS1 };       // conv_igemm_kernel, conv3x3_lds_kernel, conv1x1_stream_kernel, conv3x3_ws_kernel, conv1x1_ws_kernel
struct WsGeom { int TH, TW, tiles_x, tiles_y, total_tiles, pitch, nchunks, nwc, nwp; };
struct Ws1Geom { int npx, total_tiles, pitch, nwc, nwp; };
struct ConvPlan {
    int kind;                       // ConvKind
    int ct, pt, ksplit;             // channel tiles / pixel tiles per wave (CONV_WS1: pixel tiles per workgroup); split-K ways
    int fastk;                      // 3x3 with K a multiple of the k-step
    int wres, rowt, tpw1;           // CONV_LDS: resident weights; CONV_WS: row-tile form, 64 -> 64 as 4 waves x one tile
    const void* fn[2];              // kernel(s); fn[1]: CONV_WS's second launch for an odd last channel tile, else null
    unsigned gx, gy;                // grid (256 threads per workgroup)
    unsigned lds;                   // dynamic LDS bytes
    int tiles_x, tiles_per_img, total_tiles;    // CONV_LDS
    int ngroups;                    // CONV_STREAM
    int tiles0;                     // CONV_WS: channel tiles the first launch covers
    WsGeom ws;                      // CONV_WS (of the first launch)
    Ws1Geom ws1;                    // CONV_WS1
};
void       conv_plan(int dtype, int ks, const ConvArgs& a, const Switches& sw, ConvPlan* plan);
hipError_t launch_conv(const ConvArgs& a, const ConvPlan& plan, hipStream_t s);
hipError_t conv_init();
// the 80 -> 80 class-branch convs: weight-stationary with K packed across taps (kernels_conv.hip: conv3x3_wsk_kernel); weights tiled with cin_store = 80
struct WskPlan { WsGeom g; unsigned gx, lds; };
bool       conv_wsk_ok(const ConvArgs& a, const Switches& sw, WskPlan* plan);     // does launch_conv_wsk take this launch?  (fills the plan if so)
hipError_t launch_conv_wsk(const ConvArgs& a, const WskPlan& plan, hipStream_t s);
int        conv_kstep(int dtype);
// a 64-channel bottleneck's two 3x3 convs as one weight-stationary launch (kernels_conv.hip: conv3x3_ws_pair_kernel); the intermediate map stays in LDS
struct WsPairArgs {
    const void* in;  int in_cs, in_co;        // x (NHWC view)
    const void* wA;  const float* bA;         // first conv: weights as the generic convs tile them ([4 tiles][18 k-steps][lane][8], pair-permuted rows)
    const void* wB;  const float* bB;         // second conv
    int H, W, n;
    void* out;       int out_cs, out_co;
    const void* res; int res_cs, res_co;      // the RES instantiation: added to the output after the activation (the bottleneck's shortcut)
    void* mid;       int mid_cs, mid_co;      // debug taps: the first conv's output view, written as well when set (null: the map stays in LDS)
};
struct WsPairGeom { int TH, TW, tiles_x, tiles_y, total_tiles; };
struct WsPairPlan { WsPairGeom g; unsigned gx, lds; const void* fn; };
// do convs a, b (their own launches planned as pa, pb) run as one pair launch?  Only where both would be the weight-stationary kernel; fills the plan if so
bool       conv_ws_pair_plan(const ConvArgs& a, const ConvArgs& b, const ConvPlan& pa, const ConvPlan& pb, const Switches& sw, WsPairPlan* plan);
hipError_t launch_conv_ws_pair(const ConvArgs& a, const ConvArgs& b, const WsPairPlan& plan, bool dump, hipStream_t s);

// kernels_pair.hip -- a C2f bottleneck (two 3x3 convs, c -> c -> c, optional shortcut) as one kernel; bf16, c = 16 / 32
struct PairArgs {
    const void* in;  int in_cs, in_co;        // x (NHWC view); also the shortcut source
    void* out;       int out_cs, out_co;
    const void* wA;  const float* bA;         // first conv: weights tiled [c/16][9][lane][frag] (frag = 8 bf16, or 4 for c = 16)
    const void* wB;  const float* bB;         // second conv
    int H, W, n;
    int TH, TW, tiles_x, tiles_y, total_tiles;
    int res;                                  // 1 = add x to the output (after the activation)
};
struct PairPlan { int th, tw, tiles_x, tiles_y, total_tiles, grid, lds_bytes; };
bool       pair_plan(int c, int n, int H, int W, const Switches& sw, PairPlan* plan);
hipError_t pair_init();
hipError_t launch_pair(int c, const PairArgs& a, const PairPlan& plan, hipStream_t s);

// a C2f block around one bottleneck as one kernel (kernels_pair.hip: c2f_kernel); mode bit 0 = cv1 in front, bit 1 = cv2 behind
struct C2fArgs {
    const void* x;  int x_cs, x_co;           // cv1 input (NHWC view); with x2 set: the half-size tensor of a fused Upsample+Concat
    const void* x2; int x2_cs, x2_co, split_c;
    const void* w1; const float* b1; int nk1; // cv1: tiled [2C/16][nk1][lane][8] (k-steps of 32); C = 16: rows in channel order, C = 32: pair-permuted
    void* cat; int cat_cs;                    // the C2f's concat buffer in HBM: [y0 | y1 | y2 | ...], C channels each
    int pair_in_co, pair_out_co;              // channel offsets of the bottleneck's input / output inside cat
    const void* wA; const float* bA; const void* wB; const float* bB; int res;     // the bottleneck (as PairArgs)
    const void* w2; const float* b2; int nk2, Cout2;   // cv2: tiled [Cout2/16][nk2][lane][frag], k-steps of C in concat order, pair-permuted rows
    void* out; int out_cs, out_co;
    int H, W, n;
    int TH, TW, tiles_x, tiles_y, total_tiles;
    int dump;                                 // also write the intermediates that would stay in LDS to cat (debug taps)
    void* mid; int mid_cs;                    // c = 64 with dump: the bottleneck's intermediate map (its first conv's output buffer of the unfused path)
};
struct C2fPlan { int th, tw, tiles_x, tiles_y, total_tiles, grid, lds_bytes, nw; };      // nw: waves per workgroup the plan was made for
bool       c2f_plan(int c, int mode, int nk1, int nk2, int cout2, int n, int H, int W, const Switches& sw, C2fPlan* plan);
hipError_t c2f_init();
hipError_t launch_c2f(int c, int mode, const C2fArgs& a, const C2fPlan& plan, hipStream_t s);
// kernels_c2f64.hip -- the same for c = 64 (c2f64_kernel: 3x3 weights in registers, 1x1 weights streamed through LDS); reached through c2f_plan / launch_c2f
bool       c2f64_plan(int mode, int nk1, int nk2, int cout2, int n, int H, int W, const Switches& sw, C2fPlan* plan);
hipError_t c2f64_init();
hipError_t launch_c2f64(int mode, const C2fArgs& a, const C2fPlan& plan, hipStream_t s);

// kernels_misc.hip
// v (here and in the two stem launchers): which instantiation of the front kernel runs (front_variants.h); with view set, n ViewRec lie behind the n descriptors
hipError_t launch_preprocess(int dtype, const uint8_t* src, const FrameDesc* desc, int n,
                             void* out_nhwc8, float* out_nchw_f32, int tw, int th, hipStream_t s, FrontVariant v);
hipError_t launch_nchw_to_nhwc8(int dtype, const float* in_nchw, void* out_nhwc8, int n, int tw, int th, hipStream_t s);
hipError_t launch_sppf_pool(int dtype, void* buf, int cs, int c, int n, int H, int W, hipStream_t s, int six_pass = 0);      // six_pass: sppf_pool_kernel also on maps of <= 16 x 16 pixels (tests / A-B)
bool       sppf_pool16_ok(int dtype, int cs, int c, int n, int H, int W, int six_pass);                        // does launch_sppf_pool take sppf_pool16_kernel?
hipError_t launch_tap_to_nchw(int dtype, const void* in, int cs, int co, int C, int H, int W, int idx, float* out, hipStream_t s);

// kernels_area.hip -- the area-average resize filter (ZLY_FLAG_AREA) as a pre-pass: the call's n request frames (src, desc; with view set, n ViewRec lie
// behind the n descriptors) -> n model-sized tight BGR frames at out ([n][th][tw][3]; lb: the letterbox geometry, padding included)
hipError_t launch_area(const uint8_t* src, const FrameDesc* desc, int n, bool view, uint8_t* out, int tw, int th, bool lb, int num_cus, hipStream_t s);

// kernels_stem.hip -- preprocess fused into the stem conv (bf16, 16-channel stem)
struct StemArgs {
    const uint8_t* src; const FrameDesc* desc;
    const void* wgt; const float* bias;       // stem weights tiled with cin_store = 4 (k = tap*4 + c), 2 k-steps
    void* out; int out_cs, out_co;
    int tw, th, Ho, Wo, Cout, tiles_x;
};
hipError_t launch_stem_fused(const StemArgs& a, int n, hipStream_t s, FrontVariant v);
int stem_tiles_x(int Wo);
// preprocess + model.0 + model.1 in one kernel (the stem map stays in LDS); st.out is only written with dump = 1 (debug taps)
struct Stem1Args {
    StemArgs st;
    const void* w1; const float* b1;          // model.1 weights tiled [2][9 taps][lane][4] (k = ci per tap, pair-permuted rows), bias in channel order
    void* out1; int out1_cs, out1_co;
    int H1, W1;                               // model.1 output map
    int TH, TW, tiles_x, tiles_y;
    int dump;
    int nw, var;                              // waves per workgroup (0 = default), kernel variant (2 = persistent workgroups + input prefetch, 1 = one tile per workgroup, 0 = round 3's staging / tap order)
    int n;                                    // frames (set by launch_stem_model1)
    int pgrid;                                // var 2: workgroups of the persistent grid (0 = as many as stay resident)
    int small_tiles;                          // 1: launch_stem_model1 halves the tile for launches with fewer workgroups than the chip holds (small batches)
    // set by launch_stem_model1 (host IEEE divides: the kernel used to spend six fp32 divides per thread on them)
    float inv_pw, inv_rw, inv_tw, inv_qb;     // 1 / patch row pitch, 1 / region width, 1 / tile width, 1 / quad blocks per patch row
    const void* wgt0p;                        // stem weights in the tap order of the conflict-free fragment reads (kernels_stem.hip: STEM1_TAP_SLOT)
};
void       stem1_plan(int H1, int W1, const Switches& sw, int* th, int* tw);
hipError_t stem1_init();
hipError_t launch_stem_model1(const Stem1Args& a, int n, hipStream_t s, FrontVariant v);
const int* stem1_tap_slot();              // [9]: k slot of tap ky * 3 + kx in Stem1Args::wgt0p (weights.h: repack_conv's tap_slot)

// kernels_sppf.hip -- SPPF (cv1 -> three 5x5 max pools -> cv2 over the concat) as one kernel; bf16, hidden width 128, maps of up to 176 pixels
struct SppfArgs {
    const void* x; int x_cs, x_co, Cin;       // cv1 input (NHWC view)
    const void* w1; const float* b1;          // cv1: tiled [c/16][Cin/32][lane][8], pair-permuted rows
    const void* w2; const float* b2;          // cv2: tiled [Cout/16][4c/32][lane][8], k in concat order [y | p1 | p2 | p3], pair-permuted rows
    void* out; int out_cs, out_co, Cout;
    void* cat; int cat_cs;                    // the block's concat buffer in HBM: written only with dump (debug taps)
    int H, W, n, c;
    int split;                                // workgroups per frame (2 / 4: sppf_split)
    int dump;
};
bool       sppf_fused_ok(const SppfArgs& a);     // does launch_sppf_fused take this launch?
int        sppf_split(int cout, int n, const Switches& sw);
hipError_t sppf_init();
hipError_t launch_sppf_fused(const SppfArgs& a, hipStream_t s);

// kernels_head.hip -- fused Detect head (final 1x1 convs + DFL + dist2bbox + sigmoid + decode/threshold)
struct HeadLevel {
    const void* box_in; const void* cls_in;   // [n][H*W][cs] activations of the two branches' second 3x3 convs
    int box_cs, cls_cs, box_cin, cls_cin;
    const void* wb; const void* wc;           // final 1x1 weights, tiled in MFMA lane order
    const float* bb; const float* bc;         // biases (padded to 16)
    int nkb, nkc;                             // k-steps of the two GEMMs
    int H, W, hw, stride_px, anchor_off, block0;
    float* logits; int logits_cs;             // optional fp32 [n][H*W][logits_cs] dump (debug taps), or null
    // box_mode != 0 (bf16; set per launch by the planner, engine.cpp: tail_box_mode): box_in is not cv2.L.1's output but its INPUT, the box half of the level's
    // Detect stem buffer (box_cs = that buffer's pixel pitch), and a wave that survives the early-out computes the 64 -> 64 3x3 conv for its own 16 anchors
    // (kernels_head.hip: tail_box_conv) in the k-step order of the dense kernel it stands in for: 1 = conv3x3_ws_kernel's, 2 = conv3x3_lds_kernel's
    int box_mode;
    const void* w1; const float* b1;          // cv2.L.1's weights as the dense op tiles them ([4 tiles][18 k-steps][lane][8], pair-permuted rows) and its bias
    void* box2;                               // debug taps: the conv's output [n][H*W][64] is written as well when set
};
#define HEAD_KMAX 8                           // most k-steps of one Detect branch the fused tail holds in registers (bf16: 256 channels, fp32: 128)
#define HEAD_WAVES 8                          // waves per workgroup of the fused Detect tail, one 16-anchor tile each
#define HEAD_GROUP (HEAD_WAVES * 16)          // anchors per workgroup; HeadLevel::block0 / total_blocks count these groups
struct HeadArgs {
    HeadLevel lv[3];
    int nc, N_total, total_blocks;
    int only_level;                           // -1: all three levels in one launch; 0..2: that level only (its own launch, beside the neck)
    float* head;                              // [n][4+nc][N_total] or null
    const FrameDesc* desc; float conf_thr;
    float skip_logit;                         // set by launch_head_fused: class logit below which no score reaches conf_thr
    int diag;                                 // diagnostic builds only (tools/head_bench.hip); 0 in the product
    struct Cand* cand; int* cand_count;
    int buf32;                                // set by launch_head_fused: every level's branch tensors are below 2 GiB -> fragments by buffer loads (lane mask as an out-of-range offset)
    int lb_tw, lb_th;                         // letterbox engine: the model size (boxes are mapped out of the letterbox, kernels_lb.hip's instantiations); 0 = stretch
};
hipError_t launch_head_fused(int dtype, const HeadArgs& a, int n, hipStream_t s);

// kernels_post.hip
struct Cand { float x, y, w, h; float conf; int cls; int anchor; int pad_; };   // 32 bytes
hipError_t launch_decode(const float* head, int nc, int N, int n, const FrameDesc* desc, float conf_thr,
                         Cand* cand, int* cand_count, hipStream_t s);
hipError_t nms_init();
hipError_t launch_nms(const Cand* cand, int* cand_count, int N, int n, float iou_thr, int nc,
                      Cand* scratch, void* slabs, int cap, uint32_t tag0, hipStream_t s, int force_general = 0);

// ---- tracking (kernels_track.hip; the rule and the step: include/zly.h) ----
#define ZLY_TRACK_MAX 64          // slots per stream as stored (max_tracks <= 64: one lane per slot)
// The track table of one stream in HBM, structure of arrays: lane t of track_kernel's wave loads and stores element t of every array.
// With max_tracks T < 64 the slots at and beyond T take no part: the tracking kernels store their live flag as 0 and every other field as they loaded
// it, and the plan kernel of the zoom regions reads them as not live (tests/test_gpu_track_tables.py pins both).
struct TrackStream {
    uint32_t frame_no, next_id, evictions, pad_;
    uint32_t live[ZLY_TRACK_MAX];
    float x[ZLY_TRACK_MAX], y[ZLY_TRACK_MAX], w[ZLY_TRACK_MAX], h[ZLY_TRACK_MAX];
    int32_t cls[ZLY_TRACK_MAX];
    uint32_t id[ZLY_TRACK_MAX], last_seen[ZLY_TRACK_MAX];
};
// The motion model's state of one stream (zly_track_motion_enable), an array of its own beside TrackStream: velocities in normalised units per frame
// of the stream, and the number of frames the track has been seen in (1 at birth).
struct TrackMotion {
    float vx[ZLY_TRACK_MAX], vy[ZLY_TRACK_MAX];
    uint32_t hits[ZLY_TRACK_MAX];
};
// grp (device, int32): [0] = S, the number of distinct streams of the call; [1 .. S + 1] = segment offsets into the frame list; [S + 2 .. 2S + 1] = the
// segments' stream indices; [2S + 2 ...] = the call's tracked frame indices ordered by (first occurrence of their stream, index).  One workgroup per segment.
hipError_t launch_track(TrackStream* states, const int* grp, int n_seg, void* slabs, int cap, int max_tracks, float match_iou, uint32_t max_lost, hipStream_t s);
// all slots of streams [first, first + count) free, frame_no = 0, evictions = 0; next_id = first_id unless that is 0
hipError_t launch_track_reset(TrackStream* states, int first, int count, uint32_t first_id, hipStream_t s);
// launch_track with the motion model (track_motion_kernel); motion[i] is the state of states[i]
hipError_t launch_track_motion(TrackStream* states, TrackMotion* motion, const int* grp, int n_seg, void* slabs, int cap, int max_tracks, float match_iou,
                               uint32_t max_lost, float beta, float v_max, hipStream_t s);
// vx = vy = 0, hits = 0 in every slot of streams [first, first + count)
hipError_t launch_track_motion_reset(TrackMotion* motion, int first, int count, hipStream_t s);

// ---- merging the slabs of a surface's tiles (kernels_merge.hip; the rule and the step: include/zly.h, "Tiles") ----
#define ZLY_MERGE_TILE_INTS 7     // a member of the tile table: source slab, x0, y0, w, h, W, H
// merge_kernel's dynamic LDS holds up to ZLY_MERGE_MAX_CANDIDATES candidates (132 KB): opted in at an engine's first merge, outside capture
hipError_t merge_init();
// tab (device, int32): [0 .. G] = the G groups' offsets into the member list; then ZLY_MERGE_TILE_INTS per member, a group's members in ascending slab
// index.  One workgroup per group merges its members' slabs (of `slabs`) into slab g of `out`, frame_tag = tag0 + g.  max_slots: the largest
// members x cap of a group (<= ZLY_MERGE_MAX_CANDIDATES): it sizes the launch.  metric: ZLY_MERGE_IOU | ZLY_MERGE_IOS.
hipError_t launch_merge(const int* tab, int n_groups, int max_slots, const void* slabs, void* out, int cap, int metric, float thr, uint32_t tag0, hipStream_t s);

// ---- resident surfaces (kernels_surface.hip; the rule: include/zly.h, "Resident surfaces"; the band record: surface_device.h) ----
struct SurfaceJob;
// one launch: every band of `bands` (device, n_bands records, 16-byte aligned) from `stage` into `store` (16-byte aligned); no byte outside a band's rows is written
hipError_t launch_surface_patch(const uint8_t* stage, const SurfaceJob* bands, int n_bands, uint8_t* store, int num_cus, hipStream_t s);
struct SurfaceMoveBand;
// one launch of a move's bands (device, 16-byte aligned): from `store` into `store` or, for the bands that say so, into `bounce` (16-byte aligned; may be
// null if no band names it).  The caller guarantees that no band reads or writes a byte that another band of the launch writes.
hipError_t launch_surface_move(const SurfaceMoveBand* bands, int n_bands, uint8_t* store, uint8_t* bounce, int num_cus, hipStream_t s);

// ---- zoom regions (kernels_zoom.hip; the rule: include/zly.h, "Zoom regions"; the frame record and the arithmetic: zoom_device.h) ----
struct ZoomFrame;
// one launch, one wavefront per frame: plans K regions for each of the n frames of `frames` (device) from states[frame.stream] (and motion[...], or
// null: vx = vy = 0) into plan[n * K].  desc / tab non-null (a frame call): the n * (1 + K) descriptors + view records and the merge table of n groups
// of 1 + K members that the host has uploaded with every region at its fallback origin; the kernel patches the origins' offsets and x0, y0
hipError_t launch_zoom_plan(const TrackStream* states, const TrackMotion* motion, const ZoomFrame* frames, int n, FrameDesc* desc, int* tab, zly_zoom_region* plan,
                            int K, int max_tracks, int region_w, int region_h, int max_age, int class_id, hipStream_t s);

// ---- chips (kernels_chips.hip; the rule: include/zly.h, "Chips"; the frame record and the arithmetic: chip_device.h) ----
struct ChipFrame;
// two launches: chip_select_kernel (one wavefront per frame) writes header and records of the n chip slabs at `chips` from the n slabs at `slabs`
// (slab_bytes apart, capacity cap); chip_cut_kernel then cuts the chips out of the frames `frames` (device, n records) of the buffer `src`
hipError_t launch_chips(const uint8_t* src, const ChipFrame* frames, int n, const void* slabs, size_t slab_bytes, int cap, void* chips, const zly_chip_config& cfg,
                        hipStream_t s);

// ---- change map (kernels_change.hip; the rule: include/zly.h, "Change map"; the records and the arithmetic: change_device.h) ----
struct ChangeItem;
struct ChangeStream;
// change_sums_kernel: the luma sums of the cells of the n frames `frames` (device) of the buffer `src` into sums[n][ZLY_CHANGE_MAX_CELLS]; max_w, max_h:
// the largest width and height among the frames (the grid's size)
hipError_t launch_change_sums(const uint8_t* src, const ChipFrame* frames, int n, int max_w, int max_h, int cell, uint32_t* sums, hipStream_t s);
// change_pick_kernel, one workgroup per frame: sums against prev[items[i].stream] -> the stream's record in recs (change_layout apart), its state and
// its grid.  plan non-null (a zoom call): the K regions per frame that zoom_plan_kernel wrote, its frame records zf, and desc / tab as it was given them
// (either may be null); the fallback regions take the peaks
hipError_t launch_change_pick(const ChangeItem* items, int n, const uint32_t* sums, ChangeStream* state, uint32_t* prev, void* recs, const zly_change_config& cfg,
                              const ZoomFrame* zf, FrameDesc* desc, int* tab, zly_zoom_region* plan, int K, hipStream_t s);

// ---- camera motion (kernels_camera.hip; the rule: include/zly.h, "Camera motion"; the records and the arithmetic: camera_device.h) ----
struct CameraItem;
struct CameraStream;
// two launches behind launch_change_sums into `sums`: camera_search_kernel, (2R + 1) x n workgroups, writes the SAD tables of the streams items[i].stream
// in recs (camera_layout apart) from sums[i] against prev[stream]; camera_pick_kernel, one workgroup per frame, writes the records' headers, the
// streams' states and their grids
hipError_t launch_camera(const CameraItem* items, int n, const uint32_t* sums, CameraStream* state, uint32_t* prev, void* recs, const zly_camera_config& cfg, hipStream_t s);
// camera_apply_kernel, one wavefront per stream of streams[n] (device): step A on tracks[stream]
hipError_t launch_camera_apply(const int* streams, int n, const CameraStream* state, void* recs, TrackStream* tracks, int max_tracks, hipStream_t s);
// streams [first, first + count): no grid, no geometry, counter 0, pending shift 0
hipError_t launch_camera_reset(CameraStream* state, void* recs, int first, int count, hipStream_t s);

}  // namespace zly

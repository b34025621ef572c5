/*
 * zly.h -- C ABI of the MI355X-native YOLO detect engine (libzly.so).
 *
 * This is the ONLY surface that touches HIP.  Host C++ (the reference's server) binds it through
 * host/hip_inference_engine.{h,cpp}, which implements the reference's plugin interface
 * `IInferenceEngine` (reference src/inference/inference_engine.h:33-43) on top of these calls;
 * Python (tests, bench) binds it with ctypes.  Plain pointers and sizes only: no C++ or torch
 * types cross this boundary.  See INTEGRATION.md for the reference-side binding.
 *
 * Each entry point names the reference interface it replaces (paths relative to the reference):
 *
 *   zly_create / zly_destroy   OnnxInferenceEngine::initialize / shutdown + loadModel + warmupModel
 *                              src/inference/onnx_engine.cpp:67-170, 173-220, 957-1062, 919-954
 *   zly_detect                 OnnxInferenceEngine::runInference (preProcess -> Session::Run ->
 *                              postProcess/applyNMS), one frame   onnx_engine.cpp:518-646
 *   zly_detect_batch           the "dynamic batching" loop that the reference leaves as a TODO and
 *                              runs frame by frame                 onnx_engine.cpp:320-365
 *   zly_submit / zly_poll / zly_wait   OnnxInferenceEngine::submitInference + the result hand-over of its
 *                              inference thread: the asynchronous, pipelined host-to-host path
 *                                                                  onnx_engine.cpp:223-261, 315-398
 *   zly_detect_device          same path with frames already resident in HBM (no reference
 *                              counterpart; used by bench.py and the multi-GPU sharding)
 *   zly_*_view                 the same entry points on a region of a larger, possibly pitched buffer (zly_frame_view below); the reference's
 *                              client cuts its region of interest out on the CPU before it sends it   src/client/screen_capture.cpp:470-538
 *   zly_preprocess             OnnxInferenceEngine::preProcess     onnx_engine.cpp:649-700
 *   zly_forward / zly_head_tensor   Ort::Session::Run "images" -> "output0"
 *                                                                  onnx_engine.cpp:560-586
 *   zly_postprocess            OnnxInferenceEngine::postProcess + applyNMS + calculateIoU
 *                                                                  onnx_engine.cpp:758-909
 *   zly_get_stats              OnnxInferenceEngine::getStatus counters  onnx_engine.cpp:279-312
 *   zly_det                    zero_latency::Detection (40 bytes)  src/common/types.h:16-26
 *   return codes               zero_latency::ErrorCode             src/common/result.h:14-48
 *
 * Threading: one engine handle may be used from several host threads; calls on one handle are
 * serialised internally (the reference serialises Session::Run the same way, onnx_engine.cpp:577).  Enqueue sections of DIFFERENT
 * engines of a process run concurrently; only stream capture (at zly_create, and on the first synchronous call of a new batch size) and
 * device allocation / release (zly_create, zly_destroy, the first zly_submit) are alone in the process.
 * Ownership: the caller owns every host buffer for the duration of the call; the engine owns all
 * device and pinned memory.  There is NO CPU fallback: without a usable HIP device zly_create
 * fails with ZLY_ERR_SYSTEM.
 */
#ifndef ZLY_H_
#define ZLY_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* zero_latency::ErrorCode values used on this path (result.h:14-48) */
#define ZLY_OK                  0
#define ZLY_ERR_INVALID_ARGUMENT 2
#define ZLY_ERR_NOT_INITIALIZED 3
#define ZLY_ERR_INFERENCE       200
#define ZLY_ERR_MODEL_NOT_FOUND 201
#define ZLY_ERR_MODEL_LOAD      202
#define ZLY_ERR_INVALID_INPUT   203
#define ZLY_ERR_SYSTEM          300
#define ZLY_PENDING             1   /* zly_poll: the ticket's batch has not completed yet; zly_submit_try: every ring slot is busy (neither is an error) */

#define ZLY_DTYPE_FP32 0   /* fp32 activations + exact-fp32 MFMA: verification mode */
#define ZLY_DTYPE_BF16 1   /* bf16 activations/weights, fp32 accumulate: production mode */

#define ZLY_FLAG_DUMP_LOGITS 1   /* also write the fp32 logits of the six final Detect convs (debug taps
                                   "model.22.cv2.L.2" / "model.22.cv3.L.2"); off in production */
#define ZLY_FLAG_NO_HEAD_TENSOR 4 /* production: the Detect kernel decodes in registers and does not write the fp32 [4+nc][N] head tensor
                                   (the reference's ORT output, 1.2 MB per frame); zly_head_tensor / zly_forward then return 2 */
#define ZLY_FLAG_ASYNC_NMS   8   /* zly_detect_device and the pipelined zly_submit path (batches >= 16): NMS of a call runs on an engine-owned stream beside the first kernels of the
                                   NEXT call (it is 64 latency-bound workgroups).  The slabs of a call are then complete after zly_join
                                   (stream order) or zly_sync / zly_read_slabs (host), whichever comes first. */
#define ZLY_FLAG_SINGLE_CHAIN 16 /* no side streams: the whole step is one chain of launches on one stream.  For SEVERAL engines per GPU fed alternate
                                   batches (their chains overlap each other: the idle time at every kernel boundary of one is filled by the other);
                                   each such engine owns exactly one stream, so that up to three of them fit the four hardware queues ROCm gives a process by default
                                   (leave GPU_MAX_HW_QUEUES alone: 8 measured 2x SLOWER on the host-to-host path) */
#define ZLY_FLAG_NO_FUSION   2   /* run every conv as its own kernel (no fused bottleneck pairs): every zly_debug_tap is then available */
#define ZLY_FLAG_LETTERBOX    32  /* resize mode of this engine: aspect-preserving bilinear letterbox (what Ultralytics-trained models expect) instead of the
                                   reference's stretch-nearest resize; boxes come back as true normalised coordinates of the request frame.  Defined below. */

/* Letterbox resize (ZLY_FLAG_LETTERBOX).  Per engine, for a request of w x h and a model of tw x th (model_w x model_h), all in integers:
 *   Geometry.  If tw*h <= th*w the width binds: nw = tw, nh = max(1, (2*h*tw + w) / (2*w)).  Otherwise nh = th, nw = max(1, (2*w*th + h) / (2*h)).
 *     (64-bit products, / truncating: round half up.)  pad_x = (tw - nw) >> 1, pad_y = (th - nh) >> 1.  This is Ultralytics' LetterBox
 *     -- round(w*r), round(dw - 0.1) -- except where h*tw/w is exactly a half, which Python rounds to even: one pixel, on ~2 of 10 000 sizes.
 *   Sampling: half-pixel centres, 16.16 fixed point, 8-bit weights, in int32.  Per axis with source length S and content length D
 *     (w, nw or h, nh), for content index d:
 *       step = ((S << 16) + (D >> 1)) / D
 *       s    = clamp(d*step + (step >> 1) - 32768, 0, (S-1) << 16)
 *       i0   = s >> 16;  i1 = min(i0 + 1, S - 1);  a = (s >> 8) & 255
 *     and per channel of the four taps p00, p01, p10, p11 (row y0|y1, column x0|x1):
 *       v = (p00*(256-ax)*(256-ay) + p01*ax*(256-ay) + p10*(256-ax)*ay + p11*ax*ay + 32768) >> 16
 *     v is a byte (255 stays 255).  Everything fits int32 for w, h <= ZLY_LETTERBOX_MAX_DIM; larger requests fail in this mode with
 *     ZLY_ERR_INVALID_INPUT (and an engine with model_w or model_h above it is refused with ZLY_ERR_INVALID_ARGUMENT).
 *   Tensor.  Model pixel (x, y) with pad_x <= x < pad_x + nw and pad_y <= y < pad_y + nh holds the B, G, R bytes v of content index
 *     (x - pad_x, y - pad_y); every other pixel holds 114, 114, 114.  Those bytes then take the stretch path exactly (/255, BGR->RGB, bf16
 *     rounding in the bf16 engine).  The convolutions' zero padding outside the tw x th tensor is unchanged.
 *   YUV frames: each of the four taps is first converted to its B, G, R bytes by the formula below, then interpolated as above.
 *   Boxes.  The head's cx, cy, bw, bh (model pixels) are mapped back with single IEEE fp32 operations (no reciprocal, no contraction):
 *       x = (cx - (float)pad_x) / (float)nw;  y = (cy - (float)pad_y) / (float)nh;  w = bw / (float)nw;  h = bh / (float)nh
 *     -- true normalised coordinates of the request frame whatever its size.  Threshold, arg-max, NMS and output order do not change.
 *   A request with w == tw and h == th has nw = tw, nh = th, no padding, step = 65536, a = 0: the map is the identity.
 * Every entry point that takes frames honours the mode; the two that take tensors and caller-supplied sizes do not: the Session::Run
 * stage keeps its model-sized input, and the postProcess stage keeps the stretch mapping (cx / img_w) on every engine. */
#define ZLY_LETTERBOX_MAX_DIM 16384

#define ZLY_FLAG_AREA         64  /* resize FILTER of this engine: the area average (box filter) over every source pixel a model pixel stands for, instead of the
                                   one pixel the stretch picks or the four the letterbox blends.  Combines with ZLY_FLAG_LETTERBOX, which remains the resize
                                   GEOMETRY.  Opt-in; a large capture reduced to the model's size no longer aliases thin and small targets in and out.  Defined below. */

/* Area resize (ZLY_FLAG_AREA).  Per engine, for a request of w x h and a model of tw x th, all in integers:
 *   Content.  Without ZLY_FLAG_LETTERBOX the request is area-resized to the content size D = (tw, th).  With it, to D = (nw, nh) of "Geometry" above,
 *     placed at (pad_x, pad_y), with 114, 114, 114 everywhere else.
 *   Per axis, with source length S (w or h), content length D and content index d, in units of 1/D of a source pixel:
 *       lo = d*S;  hi = (d+1)*S;  i0 = lo / D;  i1 = (hi - 1) / D
 *     and source index i in [i0, i1] has the weight
 *       w(d, i) = min(hi, (i+1)*D) - max(lo, i*D)
 *     -- the overlap of the content pixel's interval [lo, hi) with the source pixel's [i*D, (i+1)*D).  Interior weights equal D, the two edge weights
 *     are in 1..D, and the weights of one d sum to S.  The one definition serves S > D (a downscale), S == D (w = D at i = d alone: the identity) and
 *     S < D (it degenerates to replication with blended seams): there is no special case and no fall-back to another filter.
 *   Per channel, with the B, G, R bytes p(ix, iy) of the source pixels:
 *       acc = sum over iy of wy(y, iy) * (sum over ix of wx(x, ix) * p(ix, iy))
 *       T   = Sx*Sy
 *       v   = (acc + (T >> 1)) / T
 *     The sum is exact and / truncates: round half up.  v is a byte (255 stays 255).  acc < 255 * 2^28 needs 64 bits; everything else fits int32
 *     for w, h <= ZLY_AREA_MAX_DIM; larger requests fail in this mode with ZLY_ERR_INVALID_INPUT (and an engine with model_w or model_h above it is
 *     refused with ZLY_ERR_INVALID_ARGUMENT).
 *   Source pixels that are not BGR: every source pixel is first converted to its B, G, R bytes by the existing rules, then averaged -- YUV 4:2:0 and
 *     packed 4:2:2 by the integer conversion below with the pixel's own chroma, RGB / BGRA / RGBA as the fetch's word with X ignored.  (The decision
 *     the letterbox made for its taps.)
 *   Tensor.  The bytes v take the BGR path exactly (/255, BGR->RGB, bf16 rounding in the bf16 engine).
 *   Boxes.  Box mapping, threshold, NMS and output order do not change: an area engine maps boxes as the same engine without the flag does, from the
 *     request's w, h -- cx / w on stretch engines, the letterbox un-mapping on letterbox engines.
 *   Consequences.  A request of exactly the content size gives, bit for bit, what the engine without the flag gives.  For S = k*D the result is the
 *     k x k block mean, rounded half up.  A constant frame stays constant.  Equality with any library's INTER_AREA or BOX bytes is NOT claimed: their
 *     rounding differs.
 * Every entry point that takes frames honours the mode (the synchronous, batch, _fmt, _view, submit, device, device-view, tiled and tracked calls and
 * zly_preprocess*); zly_forward and zly_postprocess, which take tensors, do not -- the line the letterbox draws.
 * How: a pre-pass kernel writes one model-sized BGR frame per request into an engine-owned buffer of max_batch * model_w * model_h * 3 bytes (allocated
 * at zly_create only with the flag), and the engine's front kernel runs on that buffer, where its own resize is the identity.  The pre-pass lies inside
 * what zly_stats calls preprocess and is timed with the front op in zly_profile_ops; the op table of an area engine is the plain engine's. */
#define ZLY_AREA_MAX_DIM 16384

/* Pixel formats of a request frame (the *_fmt entry points; the others take ZLY_PIX_BGR).  Planes are tight: no row pitch, no padding
 * (pitched surfaces and regions of a larger buffer go through a zly_frame_view and the *_view entry points, below).
 *   ZLY_PIX_BGR          packed B,G,R, 3 bytes per pixel: nbytes = w*h*3
 *   ZLY_PIX_NV12_*       Y plane [h][w], then ONE plane of interleaved U,V pairs [h/2][w/2][2]: nbytes = w*h*3/2
 *   ZLY_PIX_I420_*       Y plane [h][w], U plane [h/2][w/2], V plane [h/2][w/2]:            nbytes = w*h*3/2
 *   ZLY_PIX_RGB          packed R,G,B, 3 bytes per pixel: nbytes = w*h*3
 *   ZLY_PIX_BGRA         packed B,G,R,X, 4 bytes per pixel: nbytes = w*h*4   (GDI 32-bit DIB, DXGI B8G8R8A8, DRM XRGB8888 / ARGB8888)
 *   ZLY_PIX_RGBA         packed R,G,B,X, 4 bytes per pixel: nbytes = w*h*4   (DXGI R8G8B8A8, DRM XBGR8888 / ABGR8888, GL_RGBA)
 *   ZLY_PIX_YUY2_*       packed 4:2:2, macropixels of two pixels Y0,U,Y1,V [h][w/2][4]: nbytes = w*h*2   (YUYV; Media Foundation / V4L2 capture)
 *   ZLY_PIX_UYVY_*       packed 4:2:2, macropixels of two pixels U,Y0,V,Y1 [h][w/2][4]: nbytes = w*h*2   (HDMI / SDI capture cards)
 * The known formats are a set, not a range: of the values between the 4:2:0 formats and ZLY_PIX_RGB, 10..13 are the packed 4:2:2 formats;
 * 5..9, 14 and 15 are unknown, reserved for further YUV layouts.
 * YUV frames (8-bit 4:2:0, limited range) need even w and h (>= 2).  Colour conversion happens in the front kernel: for the source pixel
 * (sx, sy) that the stretch-nearest resize picks (the BGR map, unchanged),
 *   Y = Yplane[sy*w + sx];  ci = (sy>>1)*(w/2) + (sx>>1);  NV12: U = UV[2ci], V = UV[2ci+1];  I420: U = Uplane[ci], V = Vplane[ci]
 * and in int32 with >> an arithmetic shift (floor):
 *   yy = max(Y-16, 0)*CY;  u = U-128;  v = V-128
 *   R = clamp((yy + CVR*v          + (1<<19)) >> 20, 0, 255)
 *   G = clamp((yy + CVG*v + CUG*u  + (1<<19)) >> 20, 0, 255)
 *   B = clamp((yy + CUB*u          + (1<<19)) >> 20, 0, 255)
 *            CY       CVR      CVG      CUG      CUB
 *   BT.601   1220542  1673527  -852492  -409993  2116026   (1.164, 1.596, 0.813, 0.391, 2.018 x 2^20)
 *   BT.709   1220945  1879825  -558796  -223607  2215014   (round(c x 2^20) from Kr = 0.2126, Kb = 0.0722, luma x 255/219, chroma x 255/224)
 * Those B,G,R bytes then take the BGR path exactly (resize map, /255, BGR->RGB): a YUV frame gives, bit for bit, what its converted BGR frame
 * gives.  Boxes stay normalised by the request's w, h.  (A letterbox engine converts each of its four taps this way, then interpolates.)
 * Packed 4:2:2 frames (YUY2 / UYVY, 8-bit, limited range) need an even w >= 2; h >= 1 has no evenness rule (chroma is not subsampled
 * vertically).  One plane; row sy holds w/2 macropixels of 4 bytes.  The fetch for the source pixel (sx, sy):
 *   m = plane0 + sy*pitch + (sx>>1)*4        (tight frame: pitch = 2*w)
 *   YUY2:  Y = m[(sx&1)*2]      U = m[1]  V = m[3]
 *   UYVY:  Y = m[1 + (sx&1)*2]  U = m[0]  V = m[2]
 * then the conversion above with the same constants.  Chroma is the pixel's own macropixel's: no interpolation between macropixels (the decision
 * 4:2:0 made).  The rule is the same: a 4:2:2 frame gives, bit for bit, what the BGR frame made of its converted pixels gives through the same
 * entry point -- same engine, same batch size and composition, stretch or letterbox (four taps converted, then interpolated).
 * Packed RGB / BGRA / RGBA frames follow THE SAME RULE: a frame of one of these formats gives, bit for bit, what the BGR frame made of its
 * B, G, R bytes gives through the same entry point -- same engine, same batch size and composition, stretch or letterbox.  The front kernel
 * fetches a pixel as the BGR fetch's word (B | G<<8 | R<<16) and everything behind the fetch is the BGR path.  Consequences: the fourth byte X
 * is never interpreted -- no alpha blending, no un-premultiplying, its value never influences a result; w, h >= 1 is the only size constraint;
 * boxes are normalised as for BGR.  The 4-byte formats are staged as they are (4/3 of a BGR frame's bytes): nothing is repacked on the host. */
#define ZLY_PIX_BGR          0
#define ZLY_PIX_NV12_BT601   1
#define ZLY_PIX_I420_BT601   2
#define ZLY_PIX_NV12_BT709   3
#define ZLY_PIX_I420_BT709   4
#define ZLY_PIX_YUY2_BT601   10
#define ZLY_PIX_UYVY_BT601   11
#define ZLY_PIX_YUY2_BT709   12
#define ZLY_PIX_UYVY_BT709   13
#define ZLY_PIX_RGB          16
#define ZLY_PIX_BGRA         17
#define ZLY_PIX_RGBA         18

/* A frame view: where a request's samples lie inside a larger buffer -- a decoder or capture surface with a row pitch, a region of interest of
 * one, a tile.  Plane offsets and line sizes as usual, with offsets from the buffer's base instead of pointers, so that one view serves host and
 * device memory alike.
 *   Planes.  The packed formats (BGR, RGB, BGRA, RGBA) and packed 4:2:2 (YUY2, UYVY) use plane 0 only; NV12 0 = Y, 1 = interleaved UV; I420 0 = Y, 1 = U, 2 = V.  Entries of
 *   planes a format does not have are ignored.
 *   Rows of plane p, with cw = w/2, ch = h/2:    packed: h rows of bpp*w bytes (bpp = 3 for BGR / RGB, 4 for BGRA / RGBA);  Y: h rows of w;
 *   NV12 UV: ch rows of 2cw;  I420 U, V: ch rows of cw;  YUY2 / UYVY: h rows of 2*w bytes.
 *   The extent of a plane is (rows-1)*pitch + row_bytes.
 *   A view is valid when fmt is known; w, h >= 1 (YUV 4:2:0: even and >= 2; packed 4:2:2: w even and >= 2, any h; the packed RGB formats have no evenness rule); every used pitch[p] >= its row bytes; every used plane's extent is < 2^31.
 *   There is no alignment requirement (a 4:2:2 macropixel's four bytes may start at any address), no negative pitch and no overlap check.
 * THE RULE: a view gives, bit for bit, what the tight frame made of its samples gives through the _fmt entry point of the same name -- same
 * engine, same batch size and composition, stretch or letterbox.  w, h of the view are the REQUEST's size for the resize map, the letterbox geometry
 * and the box normalisation: boxes come back as fractions of the region (INTEGRATION.md section 3 has the one-line map to surface coordinates).
 * Bytes of the buffer outside the region never influence a result; the engine may read those that lie inside a plane's extent (row padding,
 * neighbouring columns), and never reads a byte at or beyond off[p] + extent. */
typedef struct zly_frame_view {
    int32_t  fmt;        /* ZLY_PIX_* */
    int32_t  w, h;       /* size of the viewed region in pixels = the REQUEST's size */
    int32_t  pad_;
    uint64_t off[3];     /* byte offset from the buffer base of the region's first sample in plane p */
    int32_t  pitch[3];   /* bytes from one row of plane p to the next */
    int32_t  pad2_;
} zly_frame_view;

typedef struct zly_engine zly_engine;

/* Layout-identical to zero_latency::Detection: box{x,y,width,height}@0 (centre-x, centre-y, w, h,
 * normalised by the REQUEST's width/height, onnx_engine.cpp:802-805), confidence@16, class_id@20,
 * track_id@24, timestamp@32; sizeof == 40. */
typedef struct zly_det {
    float x, y, w, h;
    float confidence;
    int32_t class_id;
    uint32_t track_id;
    uint32_t pad_;
    uint64_t timestamp;
} zly_det;

/* Fixed-size per-frame result record left in HBM by zly_detect_device and exchanged between
 * GPUs.  n_kept may exceed cap: then only the first cap detections (in the
 * reference's output order: class asc, confidence desc) are stored and ZLY_SLAB_OVERFLOW is set. */
#define ZLY_SLAB_OVERFLOW 1u
typedef struct zly_slab_header {
    int32_t n_kept;        /* detections after NMS */
    int32_t n_candidates;  /* anchors that passed the confidence threshold */
    uint32_t flags;
    uint32_t frame_tag;    /* caller-defined (bench: global frame index) */
} zly_slab_header;
/* slab bytes = sizeof(zly_slab_header) + cap * sizeof(zly_det) */

typedef struct zly_config {
    const char* weights_path;   /* ZLYW file (ServerConfig::model_path, server/config.h:306) */
    int32_t model_w, model_h;   /* detection.model_width/height, multiples of 32 (config.h:110-149) */
    float conf_thr;             /* confidence_threshold, default 0.5 (configs/server.json:7) */
    float iou_thr;              /* nms_threshold, default 0.45 (configs/server.json:8) */
    int32_t max_batch;          /* frames per zly_detect_batch / zly_detect_device call (1..65535) */
    int32_t max_dets;           /* slab capacity per frame (cap) */
    int32_t device;             /* HIP device ordinal */
    int32_t dtype;              /* ZLY_DTYPE_* */
    int32_t warmup_runs;        /* warmupModel analogue, onnx_engine.cpp:919-954 (reference: 3): that many single-frame passes, then -- when > 0 and
                                   max_batch > 1 -- the throughput path at max_batch (graphs for batch 1 and max_batch are captured and replayed here) */
    int32_t use_graph;          /* 1: replay the forward as a hipGraph per batch size */
    int32_t flags;              /* ZLY_FLAG_* */
} zly_config;

typedef struct zly_stats {
    uint64_t inference_count;
    uint64_t inference_errors;
    double total_preprocess_ms, total_forward_ms, total_postprocess_ms;   /* device time, zly_profile_ops calls only */
    double last_detect_ms;                                                /* host wall time of the last zly_detect */
    /* production sampling (the reference accumulates its three phase timers per frame, onnx_engine.cpp:530-557,605-618):
     * every 16th call of a detect path is bracketed by hipEvents -- preprocess = the preprocess / fused preprocess+stem
     * kernel, forward = everything up to and including the Detect tail (decode + threshold are fused into it),
     * postprocess = NMS.  Sums over the sampled calls; per-frame average = sampled_*_ms / sampled_frames. */
    uint64_t sampled_frames;
    double sampled_preprocess_ms, sampled_forward_ms, sampled_postprocess_ms;
    uint64_t batches;                                                     /* calls of a detect path (any entry point) */
    uint64_t graph_replays;                                               /* of them: forward replayed as a captured hipGraph ... */
    uint64_t eager_batches;                                               /* ... or launched kernel by kernel (partial batches of the pipelined path, use_graph = 0, a capture that failed twice) */
} zly_stats;

typedef struct zly_op_info {
    char name[48];
    int32_t kind;          /* 0 preprocess, 1 conv (incl. fused upsample+concat inputs), 2 sppf-pool, 4 fused detect tail (+decode), 6 nms */
    int32_t pad_;
    double flops_per_frame;   /* 2*MAC, algorithmic */
    double bytes_per_frame;   /* algorithmic: input read once + output written once + weights */
} zly_op_info;

void    zly_default_config(zly_config* cfg);
int32_t zly_create(const zly_config* cfg, zly_engine** out);
int32_t zly_destroy(zly_engine* e);
const char* zly_last_error(void);          /* thread-local message of the last failing call */
const char* zly_version(void);

/* Bytes of one frame of format fmt (ZLY_PIX_*) and size w x h: w*h*3 for BGR / RGB, w*h*4 for BGRA / RGBA, w*h*3/2 for YUV 4:2:0, w*h*2 for packed 4:2:2; 0 for an unknown format or invalid
 * dimensions (w or h < 1; for YUV 4:2:0: odd, or < 2; for packed 4:2:2: w odd or < 2).  Host only: needs no engine and no GPU. */
size_t  zly_frame_bytes(int32_t fmt, int32_t w, int32_t h);

/* Frame views, host only (no engine, no GPU).
 * zly_view_bytes: the smallest buffer size that holds the view -- the maximum over its used planes of off[p] + extent; 0 for an invalid view.
 * zly_view_tight: the view of a tight frame as defined above (its zly_view_bytes equals zly_frame_bytes); ZLY_ERR_INVALID_ARGUMENT for an unknown
 *   format, invalid dimensions or a null output.
 * zly_view_crop: the view of the sub-rectangle (x0, y0, w, h) of a view.  Pitches stay; the offset advances by y0*pitch0 + x0*bpp in plane 0
 *   (bpp = 3 for BGR / RGB, 4 for BGRA / RGBA, 2 for YUY2 / UYVY, 1 for Y), by (y0/2)*pitch + (x0/2)*2 in the NV12 UV plane and by (y0/2)*pitch + x0/2 in the I420 chroma planes.
 *   ZLY_ERR_INVALID_ARGUMENT when the surface is invalid, the rectangle is not inside it, -- YUV 4:2:0 -- any of x0, y0, w, h is odd, or -- packed 4:2:2 -- x0 or w is odd (y0 and h may be odd).  Crops compose
 *   (out may be the surface itself). */
size_t  zly_view_bytes(const zly_frame_view* v);
int32_t zly_view_tight(int32_t fmt, int32_t w, int32_t h, zly_frame_view* out);
int32_t zly_view_crop(const zly_frame_view* surface, int32_t x0, int32_t y0, int32_t w, int32_t h, zly_frame_view* out);

/* The letterbox geometry of a w x h request in a model_w x model_h model (ZLY_FLAG_LETTERBOX, "Geometry" above): content size nw x nh and its
 * offset pad_x, pad_y inside the model tensor -- what an integrator needs to map anything else (a crosshair, a mask) between frame and model
 * space.  ZLY_OK, or ZLY_ERR_INVALID_ARGUMENT for a non-positive size or a null output.  Host only: needs no engine and no GPU. */
int32_t zly_letterbox_geometry(int32_t w, int32_t h, int32_t model_w, int32_t model_h,
                               int32_t* nw, int32_t* nh, int32_t* pad_x, int32_t* pad_y);

/* --- whole path ------------------------------------------------------------------------------ */
/* One frame, synchronous.  bgr: u8 [h][w][3] interleaved BGR in host memory, nbytes must equal
 * w*h*3 (else ZLY_ERR_INVALID_INPUT, as onnx_engine.cpp:659-665).  Writes min(n, cap) detections
 * to out and the un-capped count to *n_out. */
int32_t zly_detect(zly_engine* e, const uint8_t* bgr, size_t nbytes, int32_t w, int32_t h,
                   zly_det* out, int32_t cap, int32_t* n_out);

/* n frames (n <= max_batch), each with its own size.  out is [n][cap]; n_out is [n]. */
int32_t zly_detect_batch(zly_engine* e, int32_t n, const uint8_t* const* bgr, const size_t* nbytes,
                         const int32_t* w, const int32_t* h, zly_det* out, int32_t cap, int32_t* n_out);

/* The same with a frame format (ZLY_PIX_*): one for zly_detect_fmt, one per frame for zly_detect_batch_fmt (a batch may mix formats).
 * An unknown format fails with ZLY_ERR_INVALID_ARGUMENT; nbytes != zly_frame_bytes(fmt, w, h) (odd or too small YUV sizes included)
 * with ZLY_ERR_INVALID_INPUT.  Format ZLY_PIX_BGR is exactly zly_detect / zly_detect_batch. */
int32_t zly_detect_fmt(zly_engine* e, int32_t fmt, const uint8_t* frame, size_t nbytes, int32_t w, int32_t h,
                       zly_det* out, int32_t cap, int32_t* n_out);
int32_t zly_detect_batch_fmt(zly_engine* e, int32_t n, const int32_t* fmt, const uint8_t* const* frames, const size_t* nbytes,
                             const int32_t* w, const int32_t* h, zly_det* out, int32_t cap, int32_t* n_out);

/* The same on frame views: base / buf_bytes are the caller's whole buffer (one per frame for the batch call, with one view each).  An unknown
 * format fails with ZLY_ERR_INVALID_ARGUMENT; an otherwise invalid view, or one with zly_view_bytes above buf_bytes, with ZLY_ERR_INVALID_INPUT.
 * Letterbox engines apply ZLY_LETTERBOX_MAX_DIM to the view's w, h.  The one copy into pinned staging that the engine makes anyway takes the
 * region's rows only: PCIe and staging are charged for the region, not the surface. */
int32_t zly_detect_view(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* v, zly_det* out, int32_t cap, int32_t* n_out);
int32_t zly_detect_batch_view(zly_engine* e, int32_t n, const uint8_t* const* base, const size_t* buf_bytes, const zly_frame_view* v,
                              zly_det* out, int32_t cap, int32_t* n_out);

/* --- asynchronous, pipelined host-to-host path ------------------------------------------------------
 * The throughput path of a server: many host threads hand over frames, the engine batches them and overlaps the PCIe
 * transfers with compute.  Engine-owned ring of pinned staging slots (ZLY_STAGE_SLOTS, default 6; each holds one batch of
 * up to max_batch frames / ZLY_STAGE_MB megabytes, default 1.25 x max_batch model-sized frames):
 *   zly_submit   (any thread, concurrently) reserves a frame slot in the batch being filled and copies the pixels into
 *                pinned memory ON THE CALLING THREAD -- the one copy of the request the reference makes too
 *                (onnx_engine.cpp:233-235) -- then returns a ticket; it blocks only while every ring slot is busy.
 *   dispatch     an engine-owned thread closes the filling batch as soon as fewer than two batches are in flight (a lone
 *                frame is served at once, a backlog at full batches: no batching window), uploads it on a copy stream
 *                while the previous batch computes, runs the path, and downloads the slabs on a third stream.
 *   zly_wait     blocks until the ticket's batch is back in host memory and copies that frame's detections
 *                (min(n, cap) to out, un-capped count to *n_out; timestamps = completion time, onnx_engine.cpp:813-815);
 *                zly_poll is the non-blocking check (ZLY_OK = ready, ZLY_PENDING = not yet).
 * Every ticket must be consumed by exactly one zly_wait (its ring slot is recycled when all its tickets are); a failed
 * batch returns its error code from zly_wait for each of its tickets.  Wrong byte counts fail in zly_submit with
 * ZLY_ERR_INVALID_INPUT (onnx_engine.cpp:659-665) and produce no ticket. */
int32_t zly_submit(zly_engine* e, const uint8_t* bgr, size_t nbytes, int32_t w, int32_t h, uint64_t* ticket);
/* zly_submit that never blocks: ZLY_PENDING (no ticket, nothing copied) when every ring slot of this engine is busy.  A host that feeds
 * several engines (the plugin: one per GPU / engine instance) offers a frame to the next engine in turn and, only if that one is
 * back-pressured, to the others -- with the blocking call alone, submitting threads that all wait on one engine's ring starve the rest. */
int32_t zly_submit_try(zly_engine* e, const uint8_t* bgr, size_t nbytes, int32_t w, int32_t h, uint64_t* ticket);
/* With a frame format (ZLY_PIX_*; errors as zly_detect_fmt, no ticket then).  Each frame keeps its format through the ring: a batch may mix
 * formats.  A slot's capacity is in bytes (ZLY_STAGE_MB), so more YUV frames than BGR ones fit one. */
int32_t zly_submit_fmt(zly_engine* e, int32_t fmt, const uint8_t* frame, size_t nbytes, int32_t w, int32_t h, uint64_t* ticket);
int32_t zly_submit_try_fmt(zly_engine* e, int32_t fmt, const uint8_t* frame, size_t nbytes, int32_t w, int32_t h, uint64_t* ticket);
/* On a frame view (errors as zly_detect_view: no ticket, nothing copied).  The region's rows are copied into a tight frame of the ring. */
int32_t zly_submit_view(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* v, uint64_t* ticket);
int32_t zly_submit_try_view(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* v, uint64_t* ticket);
int32_t zly_poll(zly_engine* e, uint64_t ticket);
int32_t zly_wait(zly_engine* e, uint64_t ticket, zly_det* out, int32_t cap, int32_t* n_out);

/* n frames of identical size, contiguous in DEVICE memory ([n][h][w][3] u8).  Enqueues the whole
 * path on `stream` (a hipStream_t, NULL = the engine's own stream) and returns without
 * synchronising.  d_slabs receives n slabs of zly_slab_bytes(e) each (device memory; NULL = the
 * engine's internal slab buffer, readable with zly_read_slabs).  frame_tag0 + i is stored in
 * slab i. */
int32_t zly_detect_device(zly_engine* e, int32_t n, const void* d_frames, int32_t w, int32_t h,
                          void* d_slabs, uint32_t frame_tag0, void* stream);
/* The same for n frames of one format fmt (ZLY_PIX_*), contiguous in device memory zly_frame_bytes(fmt, w, h) apart (decoder output in HBM). */
int32_t zly_detect_device_fmt(zly_engine* e, int32_t fmt, int32_t n, const void* d_frames, int32_t w, int32_t h,
                              void* d_slabs, uint32_t frame_tag0, void* stream);
/* n frame views (a HOST array of n) of ONE device buffer d_base of buf_bytes: each frame has its own size, format, pitches and offsets, and several
 * views may lie in one surface -- tiling a large frame is one call and no copy.  The front kernel fetches through the views: nothing is staged. */
int32_t zly_detect_device_view(zly_engine* e, int32_t n, const void* d_base, size_t buf_bytes, const zly_frame_view* v,
                               void* d_slabs, uint32_t frame_tag0, void* stream);
size_t  zly_slab_bytes(const zly_engine* e);
int32_t zly_read_slabs(zly_engine* e, int32_t n, void* host_slabs);   /* syncs the engine stream */
int32_t zly_sync(zly_engine* e);
/* Make `stream` (NULL = the engine's own) wait, on the device, for the NMS of every zly_detect_device call made so far except the
 * last `lag` ones.  lag must be 0 or 1 (lag = 1: consume call k-1's slabs right after enqueuing call k); the engine keeps the
 * completion events of its last two calls only, any other lag fails with ZLY_ERR_INVALID_ARGUMENT. */
int32_t zly_join(zly_engine* e, void* stream, int32_t lag);

/* --- tracking ----------------------------------------------------------------------------------------------------------------------
 * Fills zly_det::track_id on the GPU, behind NMS.  Opt-in per engine (zly_track_enable) and per frame (its stream index): without it nothing
 * changes -- no extra launch, identical bytes, track_id = 0.  The reference's game step gives every detection with id 0 a fresh id on every frame
 * (cs16_game_adapter.cpp:243-262) and its client keys its Kalman filters by track_id (src/client/prediction_engine.cpp:19-72), so only a
 * tracked frame lets a client filter see a second measurement.  The association is the reference's own IoU matching (src/game/kalman_tracker.h,
 * threshold 0.3) without its motion model: no prediction, no min_hits, no re-identification -- the client filters what it gets.  The prediction
 * is opt-in on top of that (zly_track_motion_enable, "The motion model" below); min_hits and re-identification stay out.
 *
 * A frame may name a STREAM, an index in [0, max_streams): an ordered sequence of frames, for example one client.  The engine keeps one track
 * table per stream in HBM.
 * THE RULE: the track_ids of a stream's frames are a function of that stream's own sequence of detection lists and of nothing else -- not of
 * which other frames or streams share a call or a batch, the batch size, the entry point, whether the stream's frames arrive one per call or
 * many in one call (they are then taken in index order), or what other streams did before.  Every byte of a slab other than the track_id fields
 * equals the untracked result.
 *
 * The step for one frame of a stream.  State: frame_no (u32, starts at 0), next_id (u32, starts at 1), T = max_tracks slots
 * {live, x, y, w, h, class_id, id, last_seen}.  Input: the frame's stored detections D[0..K) in slab order, K = clamp(n_kept, 0, cap).
 *   1. frame_no += 1.
 *   2. Candidate pairs (d, t): slot t is live, D[d].class_id == slot[t].class_id and iou(D[d], slot[t]) > match_iou (strict, as in NMS); iou is
 *      calculateIoU (onnx_engine.cpp:881-909) in the same single fp32 operations, in the same order, without contraction, as NMS computes it.
 *   3. Greedy match: go through the pairs in the total order (iou descending as fp32 value, d ascending, t ascending) and accept a pair when
 *      neither its detection nor its slot has been accepted yet.  (Not the optimal assignment.)
 *   4. An accepted pair: the slot takes the detection's box, last_seen = frame_no, D[d].track_id = slot.id.
 *   5. Expiry: a live slot that was not matched in this frame and has frame_no - last_seen > max_lost (u32 arithmetic) becomes free.
 *   6. Births, for each unmatched detection in ascending d: the lowest free slot -- or, if none is free, the live slot that was neither
 *      matched nor born in this frame with the smallest last_seen, the lowest index breaking ties (one exists because T >= cap; counted as an
 *      eviction) -- becomes {live, box, class, id = next_id, last_seen = frame_no}; D[d].track_id = next_id; next_id becomes next_id + 1, or 1
 *      if that is 0.
 * So every stored detection of a tracked frame leaves with a non-zero id, and ids are per stream.
 * frame_no wraps at 2^32.  Ages (step 5, the motion model's dt, the zoom regions' age) are u32 differences and stay right across the wrap; the
 * eviction order of step 6 compares last_seen as stored, so for the few frames in which a table holds values from both sides of the wrap a slot
 * seen after it is evicted before one seen before it.  A table as stored always has 64 slots; those at and beyond T are never live, matched or born
 * into (the kernels write their live flag as 0 and leave their other fields alone).
 *
 * The motion model (zly_track_motion_enable; off by default).  Without prediction a target that moves by more than about half its width per
 * frame, or that reappears a few widths further on after a dropout, never matches its own track and gets a fresh id.  The reference's tracker
 * predicts every track to the frame's time first and matches against the predicted box (src/game/kalman_tracker.cpp:273-355, :430-460); a
 * motion engine does the same with a constant velocity per slot.  It keeps three more values per slot: vx, vy (fp32, in normalised units PER
 * FRAME OF THE STREAM) and hits (u32).  The clock is frame_no -- frames carry no timestamps on the device path -- so a stream with irregular
 * frame intervals gets a worse prediction; timestamps are out of scope.  All arithmetic is single IEEE fp32 operations in the order written,
 * without contraction, as in iou.  After step 1:
 *   P.  Predict, for every live slot: dt = frame_no - last_seen (u32); dtf = (float)dt, rounded to nearest even; px = x + vx*dtf,
 *       py = y + vy*dtf (the product is rounded first, then the sum).  The predicted box is (px, py, w, h).
 *   2'. Candidate pairs use iou(D[d], predicted box) instead of the stored box.  The class test, the strict > match_iou, the total order and
 *       the greedy acceptance (steps 2-3) do not change.
 *   4'. An accepted pair (d, t): rx = D[d].x - px, ry = D[d].y - py; g = 1.0f if hits == 1, else beta; vx = clamp(vx + g*(rx/dtf)), and
 *       likewise vy, with clamp(v) = v < -v_max ? -v_max : (v > v_max ? v_max : v); hits becomes hits + 1, saturating at 0xFFFFFFFF.  Then, as
 *       in step 4: the slot takes the detection's box, last_seen = frame_no, D[d].track_id = slot.id.
 *   5, 6. Expiry, births and the eviction order do not change.  A birth sets vx = vy = 0 and hits = 1.
 * So a track's first match takes the whole displacement as its velocity and later ones move it by beta of the residual; v_max = 0 gives the
 * plain tracker's ids bit for bit.  THE RULE holds unchanged.
 * Camera motion (zly_camera_apply_tracks, "Camera motion" below; opt-in).  THE RULE, extended: a stream's ids are a function of its own sequence
 * of detection lists and of the SHIFTS applied between them -- each one pair (nx, ny) of fp32 values added to x and y of every live slot -- and of
 * nothing else.  With the motion model on, the velocities then become SCENE-RELATIVE: a match's residual is taken against the shifted box, so
 * vx, vy hold what a target moves beyond the camera's own motion, and the prediction of step P needs the shift of the coming frame applied first.
 * Not tracked: frames that go through the synchronous host calls or the _fmt submits, and engines behind host/zly_sharded*.hpp (consecutive
 * frames of a stream land on different GPUs).  A new engine (the plugin's hot reload) starts with fresh tables. */
typedef struct zly_track_config {
    int32_t max_streams;   /* >= 1 */
    int32_t max_tracks;    /* T: max_dets <= T <= 64 (an engine with max_dets > 64 cannot track) */
    float   match_iou;     /* in [0, 1); default 0.3, kalman_tracker.h:173 */
    int32_t max_lost;      /* >= 0; default 6 = the adapter's 100 ms at the reference's 60 FPS target */
} zly_track_config;

typedef struct zly_track_state {
    uint32_t frame_no, next_id;
    int32_t  n_live;       /* live slots */
    uint32_t evictions;    /* births that found no free slot, since the stream's last reset */
} zly_track_state;

void    zly_default_track_config(zly_track_config* cfg);
/* Once per engine, before the first tracked call: allocates the tables (alone in the process, like the allocations of zly_create).  Errors --
 * ZLY_ERR_INVALID_ARGUMENT for a null or out-of-range config (see the fields) and for a second call, ZLY_ERR_SYSTEM for a failed allocation.
 * Every other tracking call on an engine without tables, a stream index below -1 or >= max_streams and a batch size outside 1..max_batch
 * fail with ZLY_ERR_INVALID_ARGUMENT and enqueue nothing. */
int32_t zly_track_enable(zly_engine* e, const zly_track_config* cfg);
/* All slots of the stream become free, frame_no and the eviction count 0; stream = -1: every stream.  first_id = 0 keeps next_id, any other value
 * sets it.  Waits for the tracking enqueued so far and takes effect before it returns; frames still waiting in the submit ring are tracked after it. */
int32_t zly_track_reset(zly_engine* e, int32_t stream, uint32_t first_id);
/* Synchronises with the tracking enqueued so far, then reads (tests, status pages). */
int32_t zly_track_state_at(zly_engine* e, int32_t stream, zly_track_state* out);

/* The motion model ("The motion model" above).  The defaults are chosen, not tuned: nobody has measured them on real footage. */
typedef struct zly_track_motion_config {
    float beta;            /* in (0, 1]: the share of a match's residual that goes into the velocity; default 0.5 */
    float v_max;           /* >= 0 and finite: |vx|, |vy| never exceed it, per frame of the stream; default 0.25 */
} zly_track_motion_config;
void    zly_default_track_motion_config(zly_track_motion_config* cfg);
/* Once per engine, after zly_track_enable: allocates the motion state (a device array of its own beside the tables), waits for the tracking
 * enqueued so far and resets every stream as zly_track_reset(e, -1, 0) does.  From then on every tracked call of the engine, on the device
 * path or the pipelined one, runs the motion step, and zly_track_reset also clears vx, vy and hits of the streams it resets.  Errors --
 * ZLY_ERR_INVALID_ARGUMENT for a null, out-of-range or NaN config, for an engine without tables and for a second call; ZLY_ERR_SYSTEM for a
 * failed allocation.  An engine that never calls it runs exactly the kernels it ran before this call existed. */
int32_t zly_track_motion_enable(zly_engine* e, const zly_track_motion_config* cfg);

/* One live slot of a stream's table.  x, y, w, h: the last matched box, not the prediction; vx, vy per frame of the stream.  On an engine
 * without the motion model vx, vy and hits are 0.  sizeof == 40. */
typedef struct zly_track {
    float    x, y, w, h, vx, vy;
    int32_t  class_id;
    uint32_t id, hits, last_seen;
} zly_track;
/* Synchronises like zly_track_state_at, then writes the stream's live slots in ascending slot order: min(n, cap) of them to out, and the
 * uncapped count n to *n_out (cap = 0 with out = NULL asks for the count alone).  frame_no - last_seen (zly_track_state_at) is a slot's
 * age: what a server needs to coast a track over frames without a detection, as the reference's predict() does. */
int32_t zly_track_read(zly_engine* e, int32_t stream, zly_track* out, int32_t cap, int32_t* n_out);

/* The device path: tracks, in place, the n slabs that the most recent zly_detect_device* call on this engine wrote.  d_slabs = NULL: the engine's
 * own slab buffer.  streams is a HOST array of n; streams[i] = -1 leaves slab i untouched, and a call with nothing but -1 launches nothing.
 * Enqueued, not synchronised: it is ordered behind that call's NMS on whichever stream the NMS ran -- with ZLY_FLAG_ASYNC_NMS the engine's NMS
 * stream, otherwise `stream` (NULL = the engine's own), which should be the stream the call was given -- and zly_join, zly_sync and
 * zly_read_slabs afterwards cover the tracking too.  A later call's kernels never overwrite slabs that the tracker still reads.
 * Slabs made elsewhere (tests) are tracked the same way on an engine that has made no call yet. */
int32_t zly_track_slabs(zly_engine* e, int32_t n, const int32_t* streams, void* d_slabs, void* stream);

/* The pipelined path: zly_submit_view / zly_submit_try_view plus the frame's stream (-1 = untracked), which rides with the frame through the ring;
 * zly_view_tight gives the view of a tight frame.  The tracker runs behind the batch's NMS, before its slabs go back to the host.  Frames of a stream
 * are tracked in ticket order; a batch may mix tracked and untracked frames.  A refused submit produces no ticket and copies nothing. */
int32_t zly_submit_view_tracked(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* v, int32_t stream, uint64_t* ticket);
int32_t zly_submit_try_view_tracked(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* v, int32_t stream, uint64_t* ticket);

/* --- Tiles -------------------------------------------------------------------------------------------------------------------------
 * Merges, on the GPU and behind NMS, the slabs that the tiles of one surface produced into one slab in surface coordinates.  A large capture
 * stretched to the model size makes a small target a few model pixels wide; sliced inference -- overlapping tiles (zly_detect_device_view takes
 * them as views of one buffer), then a merge -- is how such targets are found.  An object on a seam comes back from two or four tiles; the merge
 * maps every box to its surface and suppresses the duplicates.  Opt-in per call: an engine that never calls zly_merge_slabs or zly_detect_tiled
 * runs exactly the kernels it ran before these calls existed.
 *
 * A TILE is the rectangle (x0, y0, w, h) of a W x H surface that a slab's boxes are fractions of.  A GROUP is the set of tiles of one surface in
 * a call; a call may carry several groups (8 tiles for each of 8 clients in a batch of 64).  A whole-surface pass beside the tiles -- one more
 * view with x0 = y0 = 0, w = W, h = H -- is just another tile of its group.
 *
 * The step for one group.  Its sources are the group's slabs in ascending slab index.  All arithmetic is single IEEE fp32 operations in the
 * order written, without contraction; the (float) conversions are exact because every integer is below 2^24.
 *   1. Candidates: the stored detections of every source i, K_i = clamp(n_kept_i, 0, cap) records each.  M = sum of K_i.
 *   2. Map each candidate (x, y, bw, bh) of a tile (x0, y0, w, h) of a W x H surface to surface fractions:
 *          X = (x*(float)w + (float)x0) / (float)W        Y = (y*(float)h + (float)y0) / (float)H
 *          BW = bw*(float)w / (float)W                     BH = bh*(float)h / (float)H
 *      (the product is rounded, then the sum, then the quotient) -- the map of INTEGRATION.md section 3 and of the plugin's ZLY_CROP.
 *   3. The total order: class_id ascending (as int32), confidence descending (as fp32 value: -0 and +0 tie; a NaN confidence is outside the rule,
 *      and NMS never stores one), source slab index ascending, position in the slab ascending.
 *   4. Greedy suppression, as applyNMS (onnx_engine.cpp:837-878): go through the order; every candidate still alive suppresses every later alive
 *      candidate of the same class for which m > thr (strict).  With a the earlier and b the later candidate, on the MAPPED boxes:
 *          ax0 = a.X - a.BW/2, ay0 = a.Y - a.BH/2, ax1 = a.X + a.BW/2, ay1 = a.Y + a.BH/2, and b likewise
 *          lo_x = ax0 < bx0 ? bx0 : ax0;  hi_x = bx1 < ax1 ? bx1 : ax1;  lo_y, hi_y likewise
 *          dx = hi_x - lo_x;  dy = hi_y - lo_y;  ox = 0 < dx ? dx : 0;  oy = 0 < dy ? dy : 0;  inter = ox*oy
 *          area_a = a.BW*a.BH;  area_b = b.BW*b.BH
 *          ZLY_MERGE_IOU:  uni = area_a + area_b - inter;                 m = uni > 0 ? inter/uni : 0     (calculateIoU, :881-909, as NMS computes it)
 *          ZLY_MERGE_IOS:  mn = area_a < area_b ? area_a : area_b;        m = mn > 0 ? inter/mn : 0
 *      All pairs are tested, pairs from the same tile included.  Intersection over the smaller area is what removes the half box that a tile
 *      border cuts from an object its neighbour sees whole; IoU alone often leaves it.
 *   5. The group's output slab, in the engine's slab format and capacity: the survivors in the order of step 3, the first min(n_kept, cap) of
 *      them, with the mapped box, the source's confidence and class_id, and track_id = pad_ = timestamp = 0.  Header: n_kept = survivors
 *      (un-capped), n_candidates = M, ZLY_SLAB_OVERFLOW set when n_kept > cap or any source carries it, frame_tag = frame_tag0 + group.
 *      Records at or beyond the stored count are NOT written.  A group without tiles gives an empty slab (the header only).
 * Nothing else is fused: no averaging or union of matched boxes, no class-agnostic merging.
 * Out of scope: the plugin (there is no ZLY_TILES switch), the pipelined submit path, engines behind host/zly_sharded*.hpp. */
#define ZLY_MERGE_IOU 0
#define ZLY_MERGE_IOS 1
#define ZLY_MERGE_MAX_CANDIDATES 4096   /* tiles of a group x cap may not exceed it: a group's candidates are sorted in one workgroup's LDS */
typedef struct zly_tile {
    int32_t group;            /* -1: this slab takes no part */
    int32_t x0, y0, w, h;     /* the tile inside its surface, pixels */
    int32_t W, H;             /* the surface; equal for every tile of a group */
} zly_tile;
typedef struct zly_merge_config {
    int32_t metric;           /* ZLY_MERGE_IOU | ZLY_MERGE_IOS */
    float   thr;              /* in [0, 1) */
} zly_merge_config;
/* IoS at 0.5.  Chosen, not tuned: nobody has measured them on real footage. */
void    zly_default_merge_config(zly_merge_config* cfg);

/* The device path: merges the n slabs that the most recent zly_detect_device* call on this engine wrote (d_slabs = NULL: the engine's own slab
 * buffer), or slabs made elsewhere on an engine that has made no call yet (tests), as zly_track_slabs allows.  tiles is a HOST array of n, one per
 * slab; d_out receives n_groups slabs of zly_slab_bytes each (NULL: an engine-owned buffer of max_batch slabs, allocated on first use -- alone in
 * the process, like the submit ring -- and read with zly_read_merged); it must not overlap the sources.  The sources are not modified.
 * Enqueued, not synchronised, on exactly the stream zly_track_slabs would choose: the engine's NMS stream when the call's NMS was deferred
 * (ZLY_FLAG_ASYNC_NMS), otherwise `stream` (NULL = the engine's own), which waits for the call's completion event.  The call's completion events
 * move behind the merge: zly_join, zly_sync and zly_read_slabs cover it, and a following zly_track_slabs(e, n_groups, streams, d_out, stream)
 * tracks the merged slabs with no further synchronisation.  The tile table reaches the device through a ring of pinned records, as the tracker's
 * stream list does: after the first merge of an engine a call allocates nothing.
 * ZLY_ERR_INVALID_ARGUMENT, with nothing enqueued: n outside 1..max_batch or n_groups outside 1..n; a group index outside -1..n_groups-1; a
 * rectangle that is not inside its surface, has w or h < 1, or a surface with W or H >= 2^24; tiles of one group that disagree on W, H; a group
 * with tiles x cap > ZLY_MERGE_MAX_CANDIDATES; a null or out-of-range config (NaN included); a d_out that is the engine's own slab buffer. */
int32_t zly_merge_slabs(zly_engine* e, int32_t n, const zly_tile* tiles, int32_t n_groups, const zly_merge_config* cfg, void* d_slabs, void* d_out,
                        uint32_t frame_tag0, void* stream);
/* Waits for the merges enqueued so far, then copies the first n_groups slabs of the engine-owned merge buffer to the host (1..max_batch;
 * ZLY_ERR_INVALID_ARGUMENT otherwise, and on an engine that has not merged yet). */
int32_t zly_read_merged(zly_engine* e, int32_t n_groups, void* host_slabs);

/* The tiles of a W x H surface, host only (no engine, no GPU).  Per axis, with extent E, tile size T and overlap V: step = T - V (> 0); if
 * T >= E there is one tile and it spans the extent; otherwise count = ceil((E - T) / step) + 1 and origin_i = min(i*step, E - T), so that the
 * last tile is shifted back and every tile is full-sized.  even != 0 (YUV 4:2:0 surfaces): origins are rounded down to even; odd tile sizes or
 * extents are refused.  Its tiles are valid for packed 4:2:2 surfaces too: it rounds both axes where they need only x, which is stricter than needed.  Tiles come in row-major order with group = 0 and W, H filled in; min(count, cap) of them are written and *n_out is the
 * count (cap = 0, out = NULL asks for the count alone).  ZLY_ERR_INVALID_ARGUMENT: W, H outside 1..2^24-1, a tile size < 1, an overlap < 0 or
 * >= the tile size, the even rule, a null n_out, cap < 0 or a null out with cap > 0. */
int32_t zly_tile_grid(int32_t W, int32_t H, int32_t tile_w, int32_t tile_h, int32_t overlap_x, int32_t overlap_y, int32_t even, zly_tile* out,
                      int32_t cap, int32_t* n_out);

/* The synchronous host entry: one surface in host memory, detected in n tiles and merged as one group.  The surface's zly_view_bytes bytes are
 * uploaded ONCE, as zly_preprocess_view uploads them; the tiles are zly_view_crop's of `surface` on the device-view path (the front kernel
 * fetches through them: nothing is repacked), so letterbox engines and every pixel format are honoured because views are.  Every tile must have
 * W = surface->w, H = surface->h and group = 0.  Writes min(n_kept, cap) merged detections to out, in surface fractions, and the un-capped count
 * to *n_out; timestamps as zly_detect sets them.  Errors as zly_detect_view (for the surface and for every tile's view) plus those of
 * zly_merge_slabs and zly_view_crop. */
int32_t zly_detect_tiled(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* surface, int32_t n, const zly_tile* tiles,
                         const zly_merge_config* cfg, zly_det* out, int32_t cap, int32_t* n_out);

/* --- Resident surfaces -------------------------------------------------------------------------------------------------------------
 * Keeps the last frame of each capture stream in HBM, where the front kernel reads it, and takes "these rectangles changed" instead of the whole
 * frame.  Every other way of handing over a frame from host memory copies all of it into pinned staging and uploads all of it, every time; screen
 * capture knows better (DXGI desktop duplication hands out dirty rectangles with every frame, and the reference's own client computes the changed
 * region of each capture, src/client/screen_capture.cpp:394-470, use_difference_encoding).  Opt-in per engine: an engine that never calls
 * zly_surfaces_enable allocates nothing more and launches what it launched before.
 *
 * The STORE is one device allocation of max_surfaces SLOTS at a fixed stride (max_bytes_each rounded up to ZLY_SURFACE_ALIGN).  A slot that has been
 * defined holds one tight frame (the layout of zly_view_tight) of the slot's format and size.  A slot is VALID once an update has covered it whole
 * (the keyframe) since it was last defined.
 * THE RULE: after any sequence of defines and updates a slot holds, byte for byte, the tight frame obtained by applying those rectangles in call
 * order to the frame (a byte that no rectangle has written since the define is unspecified: hence the keyframe).  Detecting on it gives, bit for
 * bit, what zly_detect_device_view gives for the same frames uploaded whole -- in a call of the same engine, batch size and composition, with
 * stretch, letterbox or area resize.
 * How: the calling thread copies each rectangle's rows tight into the engine's pinned staging, one copy takes pixels and job table up, and ONE
 * launch of a patch kernel (csrc/kernels_surface.hip) writes every rectangle of the call into the store, whatever their number; it writes no byte
 * outside a rectangle.  Detection builds frame views into the store and takes the device-view path as it is.
 * Not covered: the pipelined submit ring (its slots are tight frames in a staging buffer of their own), the plugin and the wire format (a request
 * carries no rectangle), engines behind host/zly_sharded*.hpp, skipping inference for unchanged tiles (results across batch sizes are not
 * bit-identical, so it would break the rule), moves between two surfaces, and rectangles whose pixels lie in a caller's device buffer.
 *
 * MOVES (opt-in: zly_surface_moves_enable).  DXGI desktop duplication hands out, with every frame, move rectangles ("the w x h block at (sx, sy) now
 * lies at (dx, dy)": a scrolled view, a dragged window) to be applied, in order, BEFORE the dirty rectangles, and does not report a moved region as
 * dirty.  A MOVE is {surface, sx, sy, dx, dy, w, h}.  After a call with moves 0..n-1 every slot holds, byte for byte, the frame obtained by applying
 * them in index order; each move acts on every plane of the format as  tmp = copy of the source rectangle; destination rectangle = tmp  -- memmove
 * semantics: the source is read whole before the destination is written.  Both (sx, sy, w, h) and (dx, dy, w, h) must be legal for zly_view_crop on
 * the surface's tight view: inside the surface, with the format's evenness rules (4:2:0: all even; 4:2:2: x and w even).  A move whose source equals
 * its destination is legal and changes nothing.  No byte outside a destination rectangle is written, not even with its own value.  The slot must be
 * defined and valid; a move never makes a slot valid.  THE RULE extends to moves: detecting on a slot after moves gives, bit for bit, what the frame
 * so obtained gives when uploaded whole.
 * How: two moves of a call CONFLICT when they name the same surface and the source of one intersects the destination of the other, or their
 * destinations intersect.  The call is cut into consecutive PHASES in index order: a move joins the current phase unless it conflicts with a move
 * already in it, or it overlaps itself (source and destination intersect) and the bounce buffer has no room left in this phase; then it opens the
 * next phase.  A phase is at most two launches on the engine's stream: the move kernel (csrc/kernels_surface.hip) copies the moves that do not
 * overlap themselves store -> store and gathers the others into the bounce buffer, and, if anything was gathered, the patch kernel scatters the
 * bounce buffer into the store.  No launch reads or writes a byte that another workgroup of it writes.  A scroll is one phase of two launches, a
 * window dragged clear of itself one phase of one launch; a chain of n moves of which each depends on the one before it is n phases -- accepted:
 * capture APIs hand out a handful of moves per frame. */
#define ZLY_SURFACE_MAX_RECTS 1024      /* rectangles per zly_surface_update / zly_detect_delta call (chosen) */
#define ZLY_SURFACE_ALIGN     256       /* the slot stride is a multiple of it */
#define ZLY_SURFACE_STORE_MAX (1ull << 56)   /* largest store in bytes: a view's plane-0 offset rides in 56 bits of the front kernels' frame descriptor */
typedef struct zly_surface_rect {
    int32_t surface;          /* slot index */
    int32_t x0, y0;           /* where the rectangle's first pixel lies in the surface; its size and format are the source view's */
} zly_surface_rect;
typedef struct zly_roi {
    int32_t x0, y0, w, h;
} zly_roi;
/* Once per engine: allocates the store (alone in the process, like the allocations of zly_create).  ZLY_ERR_INVALID_ARGUMENT for a non-positive
 * argument, for a second call and for a store above ZLY_SURFACE_STORE_MAX bytes; ZLY_ERR_SYSTEM for a failed allocation.  Every other call of this
 * section on an engine without a store, and a slot index outside 0..max_surfaces-1, fail with ZLY_ERR_INVALID_ARGUMENT and enqueue nothing. */
int32_t zly_surfaces_enable(zly_engine* e, int32_t max_surfaces, size_t max_bytes_each);
/* Slot s now holds a tight w x h frame of format fmt, and is NOT valid: how a stream starts, changes resolution, or recovers from a lost keyframe.
 * Nothing is enqueued.  Unknown format: ZLY_ERR_INVALID_ARGUMENT; a size that is illegal for the format, or more than max_bytes_each bytes
 * (zly_frame_bytes): ZLY_ERR_INVALID_INPUT. */
int32_t zly_surface_define(zly_engine* e, int32_t s, int32_t fmt, int32_t w, int32_t h);
/* Writes n_rects rectangles (1..ZLY_SURFACE_MAX_RECTS) into the store.  Rectangle i comes from the view src_views[i] of the HOST buffer bases[i] of
 * buf_bytes[i] bytes (checked as zly_detect_view checks a view); the view gives its size and its format, which must be the surface's.  Its
 * destination is what zly_view_crop gives for (x0, y0, w, h) of the surface's tight view, and it must be legal by exactly that function's rules:
 * inside the surface, and the format's evenness of x0, y0, w, h.  Two rectangles of one call that name the same surface must be disjoint -- a caller
 * with overlapping rectangles makes two calls.  A rectangle that covers its whole surface makes it valid.
 * Ordering.  The call first WAITS, on the host, for the work enqueued so far on the engine's own stream (the pinned staging is single-buffered and is
 * reused call to call, as zly_detect_tiled reuses it); it then copies the rows, enqueues the upload and the patch kernel on the engine's own stream and
 * returns without waiting for them.  On the device the patch kernel runs behind every zly_detect_surfaces call made so far, WHICHEVER stream that call
 * was given: it never overwrites a slot that an earlier call still reads, and a later zly_detect_surfaces on any stream runs behind it.  So the loop
 * update k, detect k on a caller's stream, update k + 1, ... needs no synchronisation of the caller's; what it cannot do is overlap the host copy of
 * update k + 1 with earlier work on the ENGINE's stream (with detection on a caller's stream the two overlap).
 * ZLY_ERR_INVALID_ARGUMENT: a null argument, n_rects out of range, an undefined or out-of-range slot, an unknown or mismatching format, an illegal
 * destination, an overlap; ZLY_ERR_INVALID_INPUT: an otherwise invalid source view, or one that does not fit its buffer.  If any rectangle is
 * refused, nothing is enqueued and no slot changes. */
int32_t zly_surface_update(zly_engine* e, int32_t n_rects, const zly_surface_rect* rects, const uint8_t* const* bases, const size_t* buf_bytes,
                           const zly_frame_view* src_views);
/* Waits for the updates enqueued so far, then copies the slot's zly_frame_bytes bytes to host_out (tests, snapshots, debugging).  A defined slot
 * need not be valid.  ZLY_ERR_INVALID_ARGUMENT: a null output, an undefined slot, cap_bytes too small. */
int32_t zly_surface_read(zly_engine* e, int32_t s, void* host_out, size_t cap_bytes);
/* The device path on n resident surfaces (1..max_batch; a surface may be named more than once): enqueues and returns as zly_detect_device_view does,
 * d_slabs, frame_tag0 and stream as there, ordered behind the updates enqueued so far.  rois is NULL (whole surfaces) or a HOST array of n
 * rectangles, each legal for zly_view_crop on its surface (ZLY_ERR_INVALID_ARGUMENT otherwise): the tiles of a resident surface are one call.  A
 * surface that is not valid: ZLY_ERR_INVALID_INPUT.  The slabs may go to zly_merge_slabs and zly_track_slabs like any device-path slabs. */
int32_t zly_detect_surfaces(zly_engine* e, int32_t n, const int32_t* surfaces, const zly_roi* rois, void* d_slabs, uint32_t frame_tag0, void* stream);
/* The host-memory convenience, synchronous: the update of zly_surface_update (n_rects may be 0: nothing changed), then the n named surfaces detected
 * whole, then the read-back; out, cap and n_out as zly_detect_batch_view.  Validity is judged after the update: a call may carry its own keyframe. */
int32_t zly_detect_delta(zly_engine* e, int32_t n_rects, const zly_surface_rect* rects, const uint8_t* const* bases, const size_t* buf_bytes,
                         const zly_frame_view* src_views, int32_t n, const int32_t* surfaces, zly_det* out, int32_t cap, int32_t* n_out);

/* Moves inside resident surfaces (the rule: "MOVES" above). */
#define ZLY_SURFACE_MAX_MOVES 1024      /* moves per zly_surface_move call (chosen) */
struct zly_surface_move {     /* a struct tag only: C keeps typedef names and functions in one name space, and the call below has this name */
    int32_t surface;          /* slot index */
    int32_t sx, sy;           /* the source rectangle's first pixel */
    int32_t dx, dy;           /* the destination rectangle's first pixel */
    int32_t w, h;             /* the size of both */
};
/* Once per engine, after zly_surfaces_enable: allocates the bounce buffer of scratch_bytes bytes (alone in the process, like the other enables)
 * through which moves that overlap themselves go; 0 means one slot stride (plus 48 bytes: each plane of a move starts 16-byte aligned), which holds any
 * single move.  ZLY_ERR_INVALID_ARGUMENT for a second call
 * and for an engine without a store; ZLY_ERR_SYSTEM for a failed allocation.  An engine that never calls it allocates nothing more and launches what
 * it launched before. */
int32_t zly_surface_moves_enable(zly_engine* e, size_t scratch_bytes);
/* Applies n_moves moves (1..ZLY_SURFACE_MAX_MOVES), in index order, to the store.
 * Ordering.  As zly_surface_update: the call first WAITS, on the host, for the work enqueued so far on the engine's own stream -- the band tables of
 * its launches travel through the same single-buffered pinned staging --, then enqueues one copy of the tables and the phases' launches on the
 * engine's own stream and returns without waiting for them.  On the device its kernels are ordered exactly as the patch kernel of an update is:
 * behind every zly_detect_surfaces* call made so far, whichever stream that call was given, ahead of every later one, and in call order with
 * zly_surface_update.  One captured frame is then zly_surface_move, zly_surface_update, zly_detect_surfaces, with no synchronisation of the caller's.
 * ZLY_ERR_INVALID_ARGUMENT: a null argument, n_moves out of range, an undefined or out-of-range slot, an illegal source or destination rectangle, no
 * bounce buffer (zly_surface_moves_enable), a single move that overlaps itself and is larger than the bounce buffer; ZLY_ERR_INVALID_INPUT: a slot
 * that is not valid.  If any move is refused, nothing is enqueued and no slot changes. */
int32_t zly_surface_move(zly_engine* e, int32_t n_moves, const struct zly_surface_move* moves);

/* --- Zoom regions ------------------------------------------------------------------------------------------------------------------
 * Detects, in ONE batch, a whole surface and K full-resolution regions of it around the stream's tracked targets, merges the 1 + K slabs into one
 * and tracks it.  A large capture stretched to the model size leaves a small target a few model pixels wide; a full tile grid (zly_tile_grid) finds
 * it at a dozen or more inferences per frame, nearly all on regions with nothing in them.  The reference's client instead keeps a region of interest
 * around its current target and sends that at full resolution (use_roi_encoding, src/client/screen_capture.cpp:102-107, :470-538); here the server
 * does it from its own track tables.  The regions are PLANNED ON THE GPU, in stream order, by a one-wavefront kernel (csrc/kernels_zoom.hip) that
 * reads the stream's track table where the tracker left it and writes the regions' origins into the frame descriptors, the view records and the
 * merge's tile table: the frame needs no zly_track_read, hence no synchronisation with the previous frame's tracker, and stays enqueue-only.
 * Opt-in per engine (zly_zoom_enable): an engine that never calls it allocates nothing more and launches exactly the kernels it launched before.
 *
 * The plan for one frame.  Inputs: the stream's table as left by every tracked call enqueued before -- frame_no F and the slots, with vx, vy if the
 * engine has the motion model (vx = vy = 0 otherwise) -- and the surface size W x H, 2 <= W, H < 2^24.  All float arithmetic is single IEEE fp32
 * operations in the order written, without contraction, as in the tracker; the (float) conversions of integers are exact.
 *   1. Region size: rw = min(region_w, W & ~1), rh = min(region_h, H & ~1); xmax = (W - rw) & ~1, ymax = (H - rh) & ~1.  Origins are always even:
 *      legal for every pixel format, and stricter than the packed RGB formats need -- the decision zly_tile_grid made.
 *   2. Eligible slots: live; class_id equal to the config's, or the config's is -1; F - last_seen (u32) <= max_age; and the box fits a region:
 *      w*(float)W <= (float)rw and h*(float)H <= (float)rh (a target larger than a region gains nothing from it).
 *   3. Prediction to the coming frame, as the tracker's step P will compute it: dtf = (float)(F + 1 - last_seen) (u32 difference);
 *      px = x + vx*dtf, py = y + vy*dtf (the product is rounded first).
 *   4. Order of the eligible slots: age F - last_seen ascending; then area w*h ascending as an fp32 value (-0 and +0 tie); then slot ascending.
 *      (A NaN area is outside the rule; the tracker stores none.)
 *   5. Greedy choice: go through the order until K regions are chosen.  A slot is COVERED, and skipped, if for some region (x0, y0) already chosen
 *      px - w*0.5f >= (float)x0/(float)W and px + w*0.5f <= (float)(x0 + rw)/(float)W, and likewise in y.  Otherwise it gets a region:
 *      pxc = px > 0 ? (px < 1 ? px : 1) : 0 (a NaN gives 0); cx = (int32)(pxc*(float)W), truncating; x0 = min(max(cx - rw/2, 0), xmax) & ~1; y likewise.
 *   6. The remaining regions are FALLBACKS (slot = -1, track_id = 0): the centred window, x0 = ((W - rw)/2) & ~1, y likewise -- where a crosshair
 *      is, and what the plugin's ZLY_CROP looks at.  The batch size must be known on the host, so fallbacks are detected and merged like any region;
 *      the merge removes what they duplicate.
 *
 * The frame.  Frame i's views are batch items i*(1 + K) + j: j = 0 the whole surface, j = 1..K its regions in the order chosen; n*(1 + K) <=
 * max_batch.  Group i of the merge is those 1 + K tiles of the W x H surface; the n merged slabs (frame_tag0 + i) are tracked in place with
 * streams[i], as zly_track_slabs would.
 * THE RULE: the n slabs equal, byte for byte, what this sequence of existing calls gives on an engine in the same state: the plan above;
 * zly_view_crop of each surface for each region; zly_detect_device_view on the n*(1 + K) views in that order; zly_merge_slabs with those tiles and
 * n groups; zly_track_slabs on the merged slabs.  It holds for stretch, letterbox and area engines, for every pixel format, and with and without
 * ZLY_FLAG_ASYNC_NMS.
 * Ordering.  The plan kernel runs behind the previous call's tracking, on whichever stream that ran.  With ZLY_FLAG_ASYNC_NMS this removes the
 * overlap of call k's NMS with call k + 1's front kernels: that is inherent -- the plan needs call k's tracks.
 * Out of scope: the pipelined submit ring, the plugin, engines behind host/zly_sharded*.hpp, choosing regions from anything but tracks
 * (the fallback regions alone can follow what moved: "Change map", zly_zoom_use_change), per-region sizes, and tuning the defaults (chosen, not
 * tuned: nobody has measured them on real footage; no accuracy claim is made). */
typedef struct zly_zoom_config {
    int32_t regions;              /* K: zoom regions per frame, 1..15 (chosen; default 3) */
    int32_t region_w, region_h;   /* a region in surface pixels: even, 2..16384; default model_w, model_h (1:1: the front kernel's resize is the identity) */
    int32_t max_age;              /* >= 0: slots with frame_no - last_seen > max_age are not zoomed; default 2 (chosen, not tuned) */
    int32_t class_id;             /* -1: any class; otherwise only slots of this class (the reference's HEAD = 2, say) */
} zly_zoom_config;
typedef struct zly_zoom_region {
    int32_t  x0, y0, w, h;        /* in surface pixels */
    int32_t  slot;                /* the slot the region was chosen for; -1: a fallback */
    uint32_t track_id;            /* that slot's id; 0: a fallback */
} zly_zoom_region;
void    zly_default_zoom_config(const zly_engine* e, zly_zoom_config* cfg);
/* Once per engine, after zly_track_enable (zly_track_motion_enable is optional, before or after): allocates the plan buffers, alone in the process
 * like the tracker's.  ZLY_ERR_INVALID_ARGUMENT: a null or out-of-range config, an engine without track tables, a second call,
 * (1 + K) * max_dets > ZLY_MERGE_MAX_CANDIDATES, 1 + K > max_batch.  ZLY_ERR_SYSTEM: a failed allocation. */
int32_t zly_zoom_enable(zly_engine* e, const zly_zoom_config* cfg);
/* The frame, on n surfaces that are views of the device buffer d_base (HOST array surface_views[n]; checked as zly_detect_device_view checks a
 * view, and 2 <= w, h < 2^24).  streams is a HOST array of n, every entry >= 0 and distinct within the call (two frames of one stream would be
 * planned from the same table).  d_out receives the n merged, tracked slabs (NULL: the merge's engine-owned buffer, read with zly_read_merged).
 * Enqueued, not synchronised; `stream` as in zly_detect_device_view; zly_join, zly_sync and zly_read_merged cover all of it.  Errors: those of
 * zly_detect_device_view, zly_merge_slabs and zly_track_slabs plus the rules above.  A refused call enqueues nothing and leaves every table as it was. */
int32_t zly_detect_device_zoom(zly_engine* e, int32_t n, const void* d_base, size_t buf_bytes, const zly_frame_view* surface_views, const int32_t* streams,
                               const zly_merge_config* merge_cfg, void* d_out, uint32_t frame_tag0, void* stream);
/* The same on n resident surfaces (distinct streams; a slot index may repeat), ordered with zly_surface_update as zly_detect_surfaces is. */
int32_t zly_detect_surfaces_zoom(zly_engine* e, int32_t n, const int32_t* surfaces, const int32_t* streams, const zly_merge_config* merge_cfg, void* d_out,
                                 uint32_t frame_tag0, void* stream);
/* Stage level (tests, overlays, callers who drive the views themselves).  zly_zoom_plan runs the plan kernel alone for n (1..max_batch) frames
 * of sizes W[i] x H[i] on streams[i] (>= 0; they may repeat), synchronously, and writes n*K regions; it patches nothing.  zly_zoom_read_plan waits
 * for the most recent zoom call and writes its n*K regions (n must be that call's; ZLY_ERR_INVALID_ARGUMENT otherwise, and before any zoom call). */
int32_t zly_zoom_plan(zly_engine* e, int32_t n, const int32_t* W, const int32_t* H, const int32_t* streams, zly_zoom_region* out);
int32_t zly_zoom_read_plan(zly_engine* e, int32_t n, zly_zoom_region* out);

/* --- Chips -------------------------------------------------------------------------------------------------------------------------
 * Cuts, on the GPU and behind NMS, a fixed-size CHIP -- an area-resized crop -- out of the frame for each of a slab's detections, reading the boxes
 * where the slab lies in HBM.  Everything behind a detector wants a target's pixels: a second-stage classifier, an appearance descriptor for
 * re-identification, a thumbnail for a status page, a client overlay.  Without this the only way to them is a synchronising slab read to learn
 * where the boxes are, then -- for a resident surface -- zly_surface_read of the whole surface (8 MB for 1920 x 1080 BGRA), then a crop and a resize
 * on the host.  With it the frame stays enqueue-only.  Opt-in per engine (zly_chips_enable): an engine that never calls it allocates nothing more
 * and launches exactly the kernels it launched before.
 *
 * Inputs for one frame: a slab in the usual layout (from any zly_detect_device* call, merged by zly_merge_slabs or a zoom call, tracked or not);
 * the frame view of W x H that the slab's boxes are fractions of, in any ZLY_PIX_* format -- the request view, or the surface for merged slabs --
 * with 1 <= W, H <= ZLY_AREA_MAX_DIM; the engine's chip config.  All float arithmetic is single IEEE fp32 operations in the order written, without
 * contraction, as in the zoom plan; the (float) conversions of these integers are exact.
 *   1. K = clamp(n_kept, 0, cap).  The detections are D[0..K) in slab order.
 *   2. Detection d is ELIGIBLE when class_id == -1 || D[d].class_id == class_id.  n_eligible counts them all.
 *   3. SELECTED: the first n_chips = min(max_chips, n_eligible) eligible detections, in slab order.  Chip j belongs to the j-th of them.
 *   4. The source rectangle, per axis; shown for x with the extent W, y with H likewise:
 *          e = D.w * scale;  half = e * 0.5f;  lo = D.x - half;  hi = D.x + half
 *          c(v) = v > 0 ? (v < 1 ? v : 1) : 0          (a NaN gives 0)
 *          a = (int32)(c(lo) * (float)W);  b = (int32)(c(hi) * (float)W)          (truncating)
 *          a = min(a, W - 1);  b = min(max(b, a + 1), W);  x0 = a;  rw = b - a
 *      So every float box gives a legal rectangle with 1 <= rw <= W.  No evenness is required, for the YUV formats too.
 *   5. The chip's pixels are the area resize of "Area resize" above with source lengths S = (rw, rh) and content size D = (chip_w, chip_h).  The
 *      source pixel (ix, iy) of the filter is pixel (x0 + ix, y0 + iy) of the FRAME, converted to B, G, R by the existing per-format rules at its
 *      own position in the frame: a 4:2:0 or 4:2:2 pixel uses its own chroma sample, whatever the parity of x0, y0.  The accumulation,
 *      T = rw*rh and the round-half-up division are the same.  A rectangle smaller than the chip upscales by the same rule: no other filter.
 *   6. Layouts (zly_chip_config.layout):
 *          ZLY_CHIP_BGR8      u8 [chip_h][chip_w][3], B, G, R
 *          ZLY_CHIP_RGB_F32   float [3][chip_h][chip_w], planes R, G, B, value (float)v / 255.0f -- the division zly_preprocess performs: what a
 *                             classifier takes
 *   7. The output per frame is a CHIP SLAB: a zly_chip_header, 16 bytes; max_chips records zly_chip_rec, 32 bytes each; padding to a multiple of 256
 *      bytes; max_chips chips at a stride of the chip's bytes rounded up to 16.  zly_chip_layout reports the numbers.  NOTHING ELSE IS WRITTEN:
 *      records and chips at or beyond n_chips, the padding, and the bytes between a chip's end and its stride are untouched.
 * THE RULE: a chip equals, byte for byte, the area resize (tests/area_ref.py: area_bgr) of B[y0 : y0 + rh, x0 : x0 + rw] to chip_w x chip_h, where B
 * is the frame's BGR image by the format's rules.  A view gives what the tight frame of its samples gives; bytes outside the view never influence a
 * chip; no byte at or beyond a plane's extent is read.
 * Consequences.  A rectangle of exactly the chip's size returns the source pixels.  A constant frame gives constant chips.
 * Out of scope: frames in host memory (the synchronous calls, the pipelined ring); the plugin and the wire format; engines behind
 * host/zly_sharded*.hpp; aspect-preserving or padded chips; chips of tracks that have no detection in the frame; per-class chip sizes; any encoder;
 * and any accuracy claim -- weights and frames are synthetic, and the defaults are chosen, not tuned. */
#define ZLY_CHIP_BGR8     0
#define ZLY_CHIP_RGB_F32  1
#define ZLY_CHIPS_SRC_SLABS  0     /* d_slabs == NULL: the engine's own slab buffer */
#define ZLY_CHIPS_SRC_MERGED 1     /* d_slabs == NULL: the merge's engine-owned output (zly_merge_slabs and the zoom calls given NULL) */
typedef struct zly_chip_config {
    int32_t chip_w, chip_h;   /* 1..256; default 64, 64 (chosen, not tuned) */
    int32_t max_chips;        /* per frame, 1..max_dets; default min(max_dets, 16) */
    int32_t class_id;         /* -1: any */
    float   scale;            /* finite, in [1, 4]; default 1.25 (chosen, not tuned) */
    int32_t layout;           /* ZLY_CHIP_BGR8 (default) | ZLY_CHIP_RGB_F32 */
} zly_chip_config;
typedef struct zly_chip_header {
    int32_t  n_chips, n_eligible;
    uint32_t frame_tag;       /* copied from the slab */
    uint32_t flags;           /* 0 */
} zly_chip_header;
typedef struct zly_chip_rec {
    int32_t  det;             /* the detection's index in its slab */
    int32_t  class_id;
    uint32_t track_id;
    float    confidence;
    int32_t  x0, y0, w, h;    /* the source rectangle in frame pixels */
} zly_chip_rec;
void    zly_default_chip_config(const zly_engine* e, zly_chip_config* cfg);
/* Once per engine: allocates max_batch chip slabs and a small ring of frame records (alone in the process, like the other enables).
 * ZLY_ERR_INVALID_ARGUMENT: a null, out-of-range or NaN config, a second call; ZLY_ERR_SYSTEM: a failed allocation.  Every other call of this section
 * on an engine without chips fails with ZLY_ERR_INVALID_ARGUMENT. */
int32_t zly_chips_enable(zly_engine* e, const zly_chip_config* cfg);
/* bytes of one chip slab, the offset of chip 0 in it, and the bytes from one chip to the next (any output may be null) */
int32_t zly_chip_layout(const zly_engine* e, size_t* slab_bytes, size_t* pixels_off, size_t* chip_stride);
/* Cuts chip slab i (i < n, 1 <= n <= max_batch) from view i of the device buffer d_base (HOST array views[n]) with the boxes of slab i.  d_slabs
 * names the slabs (device memory, zly_slab_bytes apart); NULL: `source` picks the engine's buffer (ZLY_CHIPS_SRC_*); with a non-NULL d_slabs source
 * must be 0.  d_chips receives the n chip slabs (device memory, 16-byte aligned; NULL: the engine-owned buffer, read with zly_read_chips).
 * Enqueued, not synchronised, and ordered exactly as zly_track_slabs is: behind the NMS, merge and tracking enqueued so far, on whichever stream
 * those ran -- the engine's NMS stream when the call's NMS was deferred, otherwise `stream` (NULL = the engine's own), which waits for the call's
 * completion event.  The completion events move behind the chips: zly_join, zly_sync and zly_read_chips cover them, and a later call's kernels never
 * overwrite slabs that the chips still read.  The frame records reach the kernels through a ring of pinned records with one copy per call: after
 * zly_chips_enable a call allocates nothing and does not wait for the device.
 * ZLY_ERR_INVALID_ARGUMENT, with nothing enqueued: an engine without chips, n out of range, a bad source (or ZLY_CHIPS_SRC_MERGED on an engine that
 * has not merged), a null view array, an unknown format.  ZLY_ERR_INVALID_INPUT: a view that zly_detect_device_view would refuse, or W or H above
 * ZLY_AREA_MAX_DIM. */
int32_t zly_chips_device_view(zly_engine* e, int32_t n, const void* d_base, size_t buf_bytes, const zly_frame_view* views,
                              const void* d_slabs, int32_t source, void* d_chips, void* stream);
/* The same on n resident surfaces, whole (a slot index may repeat).  An undefined or invalid surface is refused as zly_detect_surfaces refuses it.
 * The call is a reader of the store: it runs behind the updates and moves enqueued so far, and the next zly_surface_update / zly_surface_move
 * cannot overwrite a surface while chips are still being cut from it. */
int32_t zly_chips_surfaces(zly_engine* e, int32_t n, const int32_t* surfaces, const void* d_slabs, int32_t source, void* d_chips, void* stream);
/* Waits for the chips enqueued so far, then copies the first n chip slabs (1..max_batch) of the engine-owned buffer to host_out. */
int32_t zly_read_chips(zly_engine* e, int32_t n, void* host_out);

/* --- Change map --------------------------------------------------------------------------------------------------------------------
 * Finds, on the GPU, WHAT MOVED between two frames of a stream: a coarse grid of luma sums per stream, kept in HBM and compared with the previous
 * frame's grid, gives a per-cell activity grid and up to max_peaks windows around the cells that changed most.  Zoom regions give a small target full
 * resolution, but only once it has a track, and a target a few model pixels wide is never found, never tracked and never zoomed: every region the
 * plan cannot fill from a track goes to the centred window.  The reference's client computes which part of its capture changed
 * (use_difference_encoding, src/client/screen_capture.cpp:394-470); here the server does it on frames that are already in HBM, without a byte
 * crossing PCIe and without a synchronisation, and a zoom call can put its fallback regions on those windows (zly_zoom_use_change).
 * Opt-in per engine (zly_change_enable): an engine that never calls it allocates nothing more and launches exactly the kernels it launched before.
 * What it is for: captures with a mostly static camera -- a desktop, a spectator or overview camera, surveillance-like footage.  When the whole scene
 * moves (a first-person camera turning) the map reports ZLY_CHANGE_GLOBAL and a zoom call behaves exactly as without it.
 *
 * Per-stream state: a grid geometry (W, H, C), the grid of the previous frame's sums, a step counter and a have_prev bit.
 * Inputs for one frame: a frame view of W x H in any ZLY_PIX_* format, 1 <= W, H <= ZLY_AREA_MAX_DIM; a stream index; the engine's change config.
 * All arithmetic is unsigned 32-bit integer arithmetic: everything below is exact (the oracle: tests/change_ref.py).
 *   1. Luma.  B is the frame's BGR image by the format's existing rules -- the image the chips rule names, every pixel with its own chroma sample.
 *      Y(x, y) = (29*B + 150*G + 77*R + 128) >> 8.
 *   2. Cells.  C = cell, one of 8, 16, 32, 64; gw = ceil(W / C), gh = ceil(H / C); cells are row-major, index = cy*gw + cx.  Cell (cx, cy) covers the
 *      pixels [cx*C, min((cx+1)*C, W)) x [cy*C, min((cy+1)*C, H)); npix is their number and S(c) the sum of Y over them.  A call whose gw*gh exceeds
 *      ZLY_CHANGE_MAX_CELLS is refused (one workgroup's grid in 32 KB of LDS; 3840 x 2160 at C = 32 is 8160 cells).
 *   3. FIRST.  ZLY_CHANGE_FIRST is set when the stream has no previous grid: after zly_change_enable or zly_change_reset, and when W, H or C differ
 *      from the stored geometry.  Then every A(c) = 0 and there are no peaks.  In every case the stream's stored grid becomes S, its geometry
 *      (W, H, C), and its counter advances by one; `step` is the counter after that (1 for the first frame after enable or reset).
 *   4. Activity.  A(c) = |S(c) - S_prev(c)|.  Cell c is ACTIVE when 16*A(c) > threshold_q4 * npix(c): threshold_q4 is in sixteenths of a luma level
 *      per pixel, and equality is not active.  n_active counts the active cells.
 *   5. GLOBAL.  If n_active * 1000 > max_active_permille * gw*gh, ZLY_CHANGE_GLOBAL is set and there are no peaks.  The activity grid is still written.
 *   6. Window size, as zoom step 1 from window_w, window_h: rw = min(window_w, W & ~1), rh = min(window_h, H & ~1); xmax = (W - rw) & ~1,
 *      ymax = (H - rh) & ~1.  Surfaces with W < 2 or H < 2 get no peaks.  The centre pixel of cell column cx is pcx = min(cx*C + C/2, W - 1); rows
 *      likewise.
 *   7. Peaks, greedily, over a set of LIVE cells that starts as the active cells.  Initial suppression (a zoom call's track regions, below): for each
 *      given rectangle (x0, y0, rw, rh) every cell whose centre pixel lies in [x0, x0+rw) x [y0, y0+rh) leaves the set.  Then, until max_peaks peaks
 *      are chosen or no cell is live: take the live cell with the largest A, on a tie the lowest index; its window is
 *      x0 = min(max(pcx - rw/2, 0), xmax) & ~1, y likewise; record {x0, y0, rw, rh, cx, cy, A}; remove the peak cell itself from the set, ALWAYS,
 *      and every cell whose centre pixel lies in the window.  (The clamp to xmax and the & ~1 can leave a peak's own centre outside its window --
 *      at rw = 2, and in the last column when W - rw is odd -- which is why the peak cell is removed unconditionally: the loop terminates.)
 *   8. The record of a stream: a zly_change_header, 32 bytes (pad = 0); max_peaks records zly_change_peak of 32 bytes each (pad = 0), of which those
 *      at or beyond n_peaks are UNTOUCHED; then the activity grid A[gw*gh], u32, with room for ZLY_CHANGE_MAX_CELLS cells, of which those at or
 *      beyond gw*gh are untouched.  zly_change_layout reports the offsets.  zly_change_enable zeroes the records.
 * Consequences.  A view gives what the tight frame of its samples gives; bytes outside the view never influence a sum; no byte at or beyond a plane's
 * extent is read; two identical frames give n_active = 0.
 *
 * Zoom (zly_zoom_use_change).  THE RULE of "Zoom regions", extended: with it on, the slabs of a zoom call equal, byte for byte, the explicit sequence
 * zly_change_device_view (or zly_change_surfaces) on the surfaces with streams[i]; the plan of "Zoom regions" steps 1-6; the FILL: step 7 above with
 * the plan's track regions (slot >= 0) as initial suppression, and peak p put on the p-th fallback region (slot == -1, in region order) until either
 * runs out -- that region's origin becomes the peak's window and its record {slot = -2, track_id = 0}; fallbacks left over keep the centred window;
 * then crops, detect, merge and track as before.  On a FIRST or GLOBAL frame nothing is filled.  streams[i] names both the track table and the
 * change map.  With it off, a zoom call enqueues exactly what it enqueues without a change map.
 * Out of scope: the pipelined submit ring, the plugin, the wire format, engines behind host/zly_sharded*.hpp, change maps of regions rather than whole
 * frames, and tuning the defaults (chosen, not tuned; weights and frames are synthetic: no accuracy claim is made). */
#define ZLY_CHANGE_MAX_CELLS 8192
#define ZLY_CHANGE_FIRST     1u
#define ZLY_CHANGE_GLOBAL    2u
typedef struct zly_change_config {
    int32_t cell;                 /* C: 8, 16, 32 or 64; default 32 */
    int32_t threshold_q4;         /* 0..4080, sixteenths of a luma level per pixel; default 32 (chosen, not tuned) */
    int32_t max_active_permille;  /* 0..1000; default 250 (chosen, not tuned) */
    int32_t max_peaks;            /* 1..15; default 3 */
    int32_t window_w, window_h;   /* even, 2..16384; default model_w & ~1, model_h & ~1 */
} zly_change_config;
typedef struct zly_change_header {
    int32_t  n_cells, n_active, n_peaks;
    uint32_t flags;               /* ZLY_CHANGE_FIRST | ZLY_CHANGE_GLOBAL */
    int32_t  gw, gh;
    uint32_t step;                /* the stream's counter */
    uint32_t pad;                 /* 0 */
} zly_change_header;
typedef struct zly_change_peak {
    int32_t  x0, y0, w, h;        /* the window in frame pixels */
    int32_t  cx, cy;              /* the peak cell */
    uint32_t activity;            /* its A */
    uint32_t pad;                 /* 0 */
} zly_change_peak;
void    zly_default_change_config(const zly_engine* e, zly_change_config* cfg);
/* Once per engine, alone in the process like the other enables: allocates max_streams (>= 1) grids and records and max_batch scratch grids.
 * ZLY_ERR_INVALID_ARGUMENT: a null or out-of-range config, max_streams < 1, a second call; ZLY_ERR_SYSTEM: a failed allocation.  Every other call
 * of this section on an engine without a change map fails with ZLY_ERR_INVALID_ARGUMENT. */
int32_t zly_change_enable(zly_engine* e, const zly_change_config* cfg, int32_t max_streams);
/* bytes of one stream's record, and the offsets of the peaks and of the activity grid in it (any output may be null) */
int32_t zly_change_layout(const zly_engine* e, size_t* rec_bytes, size_t* peaks_off, size_t* activity_off);
/* One frame for each of n streams (1 <= n <= max_batch): view i of the device buffer d_base (HOST array views[n]) is the next frame of streams[i]
 * (HOST array; 0 <= streams[i] < max_streams, distinct within the call).  Enqueued, not synchronised, on `stream` (NULL = the engine's own); the
 * change calls of an engine, zoom calls with zly_zoom_use_change among them, are ordered among themselves on whichever streams they run.  After
 * zly_change_enable a call allocates nothing and does not wait for the device.
 * ZLY_ERR_INVALID_ARGUMENT, with nothing enqueued and no stream changed: an engine without a change map, n out of range, a null array, an unknown
 * format, a stream out of range or twice.  ZLY_ERR_INVALID_INPUT: a view that zly_detect_device_view would refuse, W or H above ZLY_AREA_MAX_DIM,
 * more than ZLY_CHANGE_MAX_CELLS cells. */
int32_t zly_change_device_view(zly_engine* e, int32_t n, const void* d_base, size_t buf_bytes, const zly_frame_view* views, const int32_t* streams, void* stream);
/* The same on n resident surfaces, whole (a slot index may repeat).  An undefined or invalid surface is refused as zly_detect_surfaces refuses it.
 * The call is a reader of the store: it runs behind the updates and moves enqueued so far, and the next zly_surface_update / zly_surface_move waits
 * for it. */
int32_t zly_change_surfaces(zly_engine* e, int32_t n, const int32_t* surfaces, const int32_t* streams, void* stream);
/* Waits for the change calls enqueued so far, then copies min(cap_bytes, record bytes) of the stream's record -- header, peaks, activity grid -- to
 * host_out.  ZLY_ERR_INVALID_ARGUMENT: a stream out of range, cap_bytes below the header and the peaks. */
int32_t zly_change_read(zly_engine* e, int32_t stream, void* host_out, size_t cap_bytes);
/* Enqueued behind the change calls so far: the stream (-1: every stream) has no previous grid and its counter is 0.  The record is left as it is. */
int32_t zly_change_reset(zly_engine* e, int32_t stream);
/* on != 0: zoom calls fill their fallback regions from the change map (above).  ZLY_ERR_INVALID_ARGUMENT: an engine without zoom regions or without
 * a change map, or window_w, window_h != region_w, region_h.  A zoom call then also refuses (nothing enqueued) a stream at or beyond the change map's
 * max_streams (ZLY_ERR_INVALID_ARGUMENT) and a surface above ZLY_AREA_MAX_DIM or with more than ZLY_CHANGE_MAX_CELLS cells (ZLY_ERR_INVALID_INPUT). */
int32_t zly_zoom_use_change(zly_engine* e, int32_t on);

/* --- Camera motion -----------------------------------------------------------------------------------------------------------------
 * Estimates, on the GPU, ONE TRANSLATION between two consecutive frames of a stream -- how far the whole picture moved, as under a turning
 * first-person camera -- and moves the stream's tracks by it before the next frame is matched ("camera motion compensation").  The tracker
 * matches by IoU: a pan of more than about half a box width per frame leaves every track unmatched and every target with a fresh id, and the
 * motion model needs two matched frames before it helps, which are the frames the pan takes away; zoom regions are planned from the same
 * table, so under a pan every region sits where its target was one frame ago; and the change map reports ZLY_CHANGE_GLOBAL and steps aside.
 * The reference's tracker (src/game/kalman_tracker.cpp) has no answer to this either.  Here the estimate is a block-matching search over the
 * change map's coarse grids of luma sums of the two frames, which are already in HBM; nothing synchronises and nothing crosses PCIe.
 * Opt-in per engine (zly_camera_enable): an engine that never calls it allocates nothing more and launches exactly the kernels it launched before.
 *
 * Config: cell C, one of 8, 16, 32, 64; radius R, 1..8 cells: the search covers displacements of up to R cells per axis; max_residual_q4,
 * 0..4080, sixteenths of a luma level per pixel: a best match worse than that is LOST.
 * Per-stream state: the geometry (W, H, C); the grid of the previous frame's sums; a have_prev bit; the counter `step`; pend_x_q4, pend_y_q4
 * (int64): the shift, in sixteenths of a pixel, accumulated since it was last applied; the counters n_lost and n_applied.
 * All arithmetic is integer and exact, except the two fp32 operations of step A (the oracle: tests/camera_ref.py).
 * One frame of a stream, a frame view of W x H in any ZLY_PIX_* format:
 *   1. Grid.  S is exactly steps 1-2 of "Change map": the same luma of the format's BGR image, the same cells, gw = ceil(W / C),
 *      gh = ceil(H / C), gw*gh <= ZLY_CHANGE_MAX_CELLS.  Also required: gw >= 2R + 1 and gh >= 2R + 1.
 *   2. FIRST.  When the stream has no previous grid (after zly_camera_enable or zly_camera_reset) or W, H or C differ from the stored geometry:
 *      ZLY_CAMERA_FIRST is set, d = f = 0, sx_q4 = sy_q4 = 0, sad_min = sad_zero = 0, the pending shift is SET TO 0, there is no search and the
 *      SAD table is left untouched.  Steps 3-7 are skipped.
 *   3. Search.  The window is the cells cx in [R, gw - R), cy in [R, gh - R): whole cells all of them, because only the last column and row can
 *      be partial.  For every (dx, dy) in [-R, R]^2:  SAD(dx, dy) = sum over the window of |S(cx, cy) - S_prev(cx - dx, cy - dy)|,  a u64
 *      (255*W*H exceeds 2^32 from 16.8 M pixels on).  (dx, dy) is the displacement, in cells, of the content from the previous frame to this one.
 *   4. Best: the candidate least in the order (SAD ascending, |dx| + |dy| ascending, dy ascending, dx ascending).  A flat or unchanged scene
 *      gives (0, 0).  sad_min is its SAD, sad_zero = SAD(0, 0).
 *   5. Sub-cell, an equiangular fit per axis, in sixteenths of a cell.  On an axis where |d| = R: f = 0 and ZLY_CAMERA_CLIPPED is set.
 *      Otherwise s0 = sad_min, and sm, sp = the SADs at d - 1 and d + 1 on that axis with the other axis at its best.  If s0 = 0 or
 *      max(sm, sp) = s0: f = 0.  Otherwise num = 16*(sm - sp) (signed), den = 2*(max(sm, sp) - s0), q = min(floor(|num| / den), 8) and
 *      f = sign(num)*q.
 *   6. The shift in sixteenths of a pixel: sx_q4 = (16*dx + fx)*C, sy_q4 = (16*dy + fy)*C.
 *   7. LOST.  npix = (gw - 2R)*(gh - 2R)*C*C.  If 16*sad_min > max_residual_q4*npix (64-bit; equality is not lost), ZLY_CAMERA_LOST is set and
 *      n_lost advances; the frame then adds nothing to the pending shift.  d, f, sx_q4 and sy_q4 are still reported.
 *   8. Update.  Unless FIRST or LOST, pend += (sx_q4, sy_q4).  The stored grid becomes S, with its geometry, and `step` advances (1 for the
 *      first frame after enable or reset).
 *   9. The record of a stream, kept in HBM and zeroed by zly_camera_enable: a zly_camera_header, ZLY_CAMERA_HDR_BYTES bytes (pad = 0), written
 *      whole by every frame; then the SAD table, u64, row-major by (dy, dx): entry (dy + R)*(2R + 1) + (dx + R), with room for 17 x 17 entries,
 *      of which those at and beyond (2R + 1)^2 are UNTOUCHED.  zly_camera_layout reports sizes and offsets.
 *   A. Applying it to tracks (zly_camera_apply_tracks), for each named stream that has a geometry (a stream has none before its first frame
 *      and after zly_camera_reset; it is then skipped whole):
 *        nx = (float)pend_x_q4 / (float)(16*W),  ny = (float)pend_y_q4 / (float)(16*H)
 *      -- each an int -> float conversion rounded to nearest even (16*W is exact) and one fp32 division, without contraction.  Every LIVE slot
 *      of the stream's track table gets x = x + nx, y = y + ny.  Slots that are not live, and w, h, class, id, last_seen, frame_no and the
 *      motion model's vx, vy and hits stay as they are.  Then pend = 0 and n_applied advances: the apply writes those three fields of the
 *      record and no other byte of it.
 * The tracking section states what this means for ids and velocities ("Camera motion" there).
 * There is no integration into the zoom or track entry points: a caller composes zly_camera_surfaces -> zly_camera_apply_tracks ->
 * zly_detect_surfaces_zoom.
 * Out of scope: rotation, zoom and parallax (the estimate is one translation per frame); a pyramid for pans beyond R cells; compensating the
 * change map with the shift; the pipelined submit ring, the plugin, the wire format, engines behind host/zly_sharded*.hpp; and tuning the
 * defaults (max_residual_q4's is chosen, not tuned; weights and frames are synthetic: no accuracy claim is made). */
#define ZLY_CAMERA_MAX_RADIUS 8
#define ZLY_CAMERA_HDR_BYTES  96
#define ZLY_CAMERA_SAD_ROOM   289     /* (2*ZLY_CAMERA_MAX_RADIUS + 1)^2 entries */
#define ZLY_CAMERA_FIRST      1u
#define ZLY_CAMERA_LOST       2u
#define ZLY_CAMERA_CLIPPED    4u
typedef struct zly_camera_config {
    int32_t cell;                 /* C: 8, 16, 32 or 64; default 16 */
    int32_t radius;               /* R: 1..8 cells; default 4 */
    int32_t max_residual_q4;      /* 0..4080, sixteenths of a luma level per pixel; default 64 (chosen, not tuned) */
} zly_camera_config;
typedef struct zly_camera_header {
    uint32_t flags;               /* ZLY_CAMERA_FIRST | ZLY_CAMERA_LOST | ZLY_CAMERA_CLIPPED */
    uint32_t step;                /* the stream's counter */
    int32_t  gw, gh;
    int32_t  dx, dy;              /* the best displacement in cells */
    int32_t  fx, fy;              /* the sub-cell parts, sixteenths of a cell, -8..8 */
    int32_t  sx_q4, sy_q4;        /* this frame's shift, sixteenths of a pixel */
    uint32_t n_lost, n_applied;
    uint64_t sad_min, sad_zero;
    int64_t  pend_x_q4, pend_y_q4;
    uint32_t pad[4];              /* 0 */
} zly_camera_header;
void    zly_default_camera_config(zly_camera_config* cfg);
/* Once per engine, alone in the process like the other enables: allocates max_streams (>= 1) grids and records and max_batch scratch grids.
 * ZLY_ERR_INVALID_ARGUMENT: a null or out-of-range config, max_streams < 1, a second call; ZLY_ERR_SYSTEM: a failed allocation.  Every other call
 * of this section on an engine without the feature fails with ZLY_ERR_INVALID_ARGUMENT.  After the enable, no call of this section allocates or
 * waits for the device (the reads excepted: they wait). */
int32_t zly_camera_enable(zly_engine* e, const zly_camera_config* cfg, int32_t max_streams);
/* bytes of one stream's record, the offset of the SAD table in it and the table's room in entries (any output may be null) */
int32_t zly_camera_layout(const zly_engine* e, size_t* rec_bytes, size_t* sad_off, size_t* sad_room);
/* One frame for each of n streams (1 <= n <= max_batch): view i of the device buffer d_base (HOST array views[n]) is the next frame of streams[i]
 * (HOST array; 0 <= streams[i] < max_streams, distinct within the call).  Enqueued, not synchronised, on `stream` (NULL = the engine's own); the
 * calls of this section are ordered among themselves on whichever streams they run.  Three launches: the change map's sums kernel into the
 * camera's own scratch grids, the search, the pick.
 * ZLY_ERR_INVALID_ARGUMENT, with nothing enqueued and no stream changed: an engine without the feature, n out of range, a null array, an unknown
 * format, a stream out of range or twice.  ZLY_ERR_INVALID_INPUT: a view that zly_detect_device_view would refuse, W or H above ZLY_AREA_MAX_DIM,
 * more than ZLY_CHANGE_MAX_CELLS cells, gw or gh below 2R + 1. */
int32_t zly_camera_device_view(zly_engine* e, int32_t n, const void* d_base, size_t buf_bytes, const zly_frame_view* views, const int32_t* streams, void* stream);
/* The same on n resident surfaces, whole (a slot index may repeat).  An undefined or invalid surface is refused as zly_detect_surfaces refuses it.
 * The call is a reader of the store, with the protocol of zly_change_surfaces. */
int32_t zly_camera_surfaces(zly_engine* e, int32_t n, const int32_t* surfaces, const int32_t* streams, void* stream);
/* Waits for the calls of this section enqueued so far, then copies min(cap_bytes, record bytes) of the stream's record to host_out.
 * ZLY_ERR_INVALID_ARGUMENT: a null output, a stream out of range, cap_bytes below ZLY_CAMERA_HDR_BYTES. */
int32_t zly_camera_read(zly_engine* e, int32_t stream, void* host_out, size_t cap_bytes);
/* Enqueued behind the calls of this section so far: the stream (-1: every stream) has no previous grid and no geometry, its counter is 0 and its
 * pending shift is 0 -- pend_x_q4 and pend_y_q4 of the record are zeroed; the rest of the record, n_lost and n_applied included, is left as it is. */
int32_t zly_camera_reset(zly_engine* e, int32_t stream);
/* Step A for the n named streams (HOST array; 1 <= n <= the camera's max_streams; distinct).  Needs zly_track_enable: camera stream i is track
 * stream i, as with the change map.  Enqueued, not synchronised, on `stream` (NULL = the engine's own): behind the camera calls and the tracked
 * calls enqueued so far, on whichever streams those ran, and ahead of every later zly_track_slabs and zoom call -- on an engine with the feature
 * the tracking kernels and the zoom plan wait for the most recent apply.  One launch, one wavefront per stream.  The call takes an entry of the
 * camera's ring and one of the tracker's; like every ring of the engine, taking an entry waits for the work that used it eight calls ago.
 * ZLY_ERR_INVALID_ARGUMENT, with nothing enqueued: an engine without the feature or without track tables, a null array, n out of range, a stream
 * named twice or at or beyond either table's max_streams. */
int32_t zly_camera_apply_tracks(zly_engine* e, int32_t n, const int32_t* streams, void* stream);

/* --- stage-level entry points (parity tests) ------------------------------------------------- */
/* preProcess: out_nchw is host fp32 [3][model_h][model_w]. */
int32_t zly_preprocess(zly_engine* e, const uint8_t* bgr, size_t nbytes, int32_t w, int32_t h, float* out_nchw);
int32_t zly_preprocess_fmt(zly_engine* e, int32_t fmt, const uint8_t* frame, size_t nbytes, int32_t w, int32_t h, float* out_nchw);
/* preProcess of a frame view: the buffer's first zly_view_bytes bytes are uploaded as they are and the kernel fetches through the view. */
int32_t zly_preprocess_view(zly_engine* e, const uint8_t* base, size_t buf_bytes, const zly_frame_view* v, float* out_nchw);
/* Session::Run: images is host fp32 [n][3][model_h][model_w] (rounded to the engine dtype on
 * upload); head_out is host fp32 [n][4+nc][N]. */
int32_t zly_forward(zly_engine* e, int32_t n, const float* images_nchw, float* head_out);
/* head tensor of frame `idx` of the most recent detect/forward call: host fp32 [4+nc][N]. */
int32_t zly_head_tensor(zly_engine* e, int32_t idx, float* head_out);
/* postProcess + applyNMS on a caller-supplied head tensor (host fp32 [4+nc][N]); any nc/N. */
int32_t zly_postprocess(zly_engine* e, const float* head, int32_t num_classes, int32_t num_boxes,
                        int32_t img_w, int32_t img_h, float conf_thr, float iou_thr,
                        zly_det* out, int32_t cap, int32_t* n_out, int32_t* n_candidates);
/* copies an intermediate conv output of frame idx to the host as fp32 [C][H][W] (debug/parity);
 * name is the conv's module path, e.g. "model.4.cv2".  *c,*h,*w receive the shape. */
int32_t zly_debug_tap(zly_engine* e, const char* name, int32_t idx, float* out, size_t cap_floats,
                      int32_t* c, int32_t* h, int32_t* w);

/* --- introspection / measurement ------------------------------------------------------------- */
int32_t zly_num_classes(const zly_engine* e);
/* 1 when the model file stores its weights as fp8 e4m3 (+ per-output-channel power-of-two exponents; BASELINE configs[4]): they are
 * dequantised once at load -- exactly representable in bf16 -- and the engine computes in bf16 as with any other file */
int32_t zly_weights_fp8(const zly_engine* e);
int32_t zly_num_anchors(const zly_engine* e);
int32_t zly_num_ops(const zly_engine* e);
int32_t zly_op_info_at(const zly_engine* e, int32_t i, zly_op_info* out);
/* Launch groups: the engine fuses ops into one kernel depending on the batch size (preprocess + model.0 + model.1; whole C2f blocks;
 * bottleneck pairs; the Detect tail of all levels; merged Detect launches on the latency path).  For op i at batch size n:
 * covered_by = the op whose launch does op i's work (== i when op i launches itself; then the other fields describe that launch):
 * n_ops it covers, their summed algorithmic flops and un-fused bytes, and bytes_fused = what has to cross the launch boundary
 * (inputs not produced inside the group + outputs read outside the group + weights) -- the byte count a fused launch's HBM
 * roofline is priced against (bench.py). */
typedef struct zly_launch_info {
    int32_t covered_by;
    int32_t n_ops;
    double flops_per_frame;
    double bytes_unfused_per_frame;
    double bytes_fused_per_frame;
    double weight_bytes;              /* part of both byte counts; per launch, not per frame */
} zly_launch_info;
int32_t zly_launch_info_at(zly_engine* e, int32_t i, int32_t n, zly_launch_info* out);
/* name and tile shape of the kernel op i launches at batch size n (the engine picks kernels per launch size) */
int32_t zly_op_kernel_name(zly_engine* e, int32_t i, int32_t n, char* out, size_t cap);
/* Runs the device path `reps` times on n resident frames with a hipEvent pair around every
 * kernel launch (no graph) and writes the mean milliseconds per op to ms_out[zly_num_ops]. */
int32_t zly_profile_ops(zly_engine* e, int32_t n, const void* d_frames, int32_t w, int32_t h,
                        int32_t reps, float* ms_out);
int32_t zly_get_stats(const zly_engine* e, zly_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* ZLY_H_ */

// sppf_probe.hip -- TEST INFRASTRUCTURE (never part of libzly.so): single launches of the SHIPPED SPPF kernels on buffers the caller made.
// Linked against the very kernels_misc.o, kernels_sppf.o and weights.o that go into libzly.so (Makefile: $(OUT)/libsppf_probe.so, -Wl,-Bsymbolic
// so that its calls bind to its own copy when libzly.so lives in the same process); tests/test_gpu_sppf.py loads it with ctypes.
//   sppf_probe_pool : launch_sppf_pool (sppf_pool16_kernel / sppf_pool_kernel<bf16_t> / <float>) on the middle frames of a guarded concat buffer
//   sppf_probe_fused: launch_sppf_fused on plain fp32 [cout][cin] weights, packed here as engine.cpp's conv() packs model.9.cv1 / cv2
// Both check the launchers' documented contract on the host and return -1 WITHOUT launching for anything outside it; what lies inside the contract
// but outside a kernel's range is the launcher's to refuse (hipErrorInvalidValue), and the buffers are downloaded all the same.
#include "zly_internal.h"
#include "weights.h"
#include <stdint.h>
#include <string.h>
#include <vector>

using namespace zly;

// kernels_misc.o also holds the preprocess launcher, whose picker asks the side units (front_variants.h) for their instantiations.  Those objects are
// not linked here and no preprocess kernel is ever launched from this library: their getters answer "no such kernel".
namespace zly {
template <int TU> const void* preprocess_kernel_in(FrontVariant v, int dtype);
template <> const void* preprocess_kernel_in<ZLY_TU_LB>(FrontVariant, int) { return nullptr; }
template <> const void* preprocess_kernel_in<ZLY_TU_VIEW>(FrontVariant, int) { return nullptr; }
template <> const void* preprocess_kernel_in<ZLY_TU_PIX>(FrontVariant, int) { return nullptr; }
template <> const void* preprocess_kernel_in<ZLY_TU_PIX_VIEW>(FrontVariant, int) { return nullptr; }
}  // namespace zly

#define PROBE_TRY(x) do { hipError_t r_ = (x); if (r_ != hipSuccess && rc == hipSuccess) rc = r_; } while (0)

// buf_in / buf_out: [guard_frames + n + guard_frames][H*W][cs] elements of dtype (bf16: 2 bytes, fp32: 4), buf_bytes each.  The whole buffer is
// uploaded, launch_sppf_pool runs on the n middle frames, the whole buffer comes back.  *kernel_out = what sppf_pool16_ok said (1: sppf_pool16_kernel).
// Returns the first HIP error code (0 = hipSuccess; the launcher's hipErrorInvalidValue for a map it refuses), or -1 for arguments outside the contract.
extern "C" int sppf_probe_pool(int dtype, const void* buf_in, size_t buf_bytes, int cs, int c, int n, int H, int W, int six_pass, int guard_frames,
                               void* buf_out, int* kernel_out)
{
    if (!buf_in || !buf_out || !kernel_out) return -1;
    if (dtype != ZLY_DTYPE_BF16 && dtype != ZLY_DTYPE_FP32) return -1;
    if (c < 8 || cs < 8 || n < 1 || n > 65535 || H < 1 || W < 1 || H > 4096 || W > 4096 || guard_frames < 0 || guard_frames > 4) return -1;
    if (c % 8 != 0 || cs % 8 != 0 || (long)cs < 4L * c) return -1;
    const size_t esz = dtype == ZLY_DTYPE_BF16 ? 2 : 4;
    const size_t frame = (size_t)H * W * cs * esz;
    if (buf_bytes != frame * (size_t)(n + 2 * guard_frames)) return -1;
    *kernel_out = sppf_pool16_ok(dtype, cs, c, n, H, W, six_pass) ? 1 : 0;

    hipError_t rc = hipSuccess;
    unsigned char* d = nullptr;
    hipStream_t s = nullptr;
    PROBE_TRY(hipMalloc((void**)&d, buf_bytes));
    PROBE_TRY(hipStreamCreate(&s));
    if (rc == hipSuccess) PROBE_TRY(hipMemcpyAsync(d, buf_in, buf_bytes, hipMemcpyHostToDevice, s));
    hipError_t launched = hipSuccess;
    if (rc == hipSuccess) launched = launch_sppf_pool(dtype, d + frame * guard_frames, cs, c, n, H, W, s, six_pass);
    if (rc == hipSuccess) PROBE_TRY(hipStreamSynchronize(s));
    if (rc == hipSuccess) PROBE_TRY(hipMemcpy(buf_out, d, buf_bytes, hipMemcpyDeviceToHost));
    if (s) PROBE_TRY(hipStreamDestroy(s));
    if (d) PROBE_TRY(hipFree(d));
    return (int)(rc != hipSuccess ? rc : launched);
}

static void pack_1x1(const float* w, const float* b, int cout, int cin, std::vector<uint8_t>* wp, std::vector<float>* bp)
{
    ConvRec r;
    r.name = "probe"; r.cin = cin; r.cout = cout; r.k = 1; r.stride = 1; r.act = 1;
    r.w.assign(w, w + (size_t)cout * cin);
    r.b.assign(b, b + cout);
    int cout_total = 0, cout_pad = 0, nk = 0;
    repack_conv({&r}, cin, 32, true, wp, bp, &cout_total, &cout_pad, &nk, true);      // engine.cpp conv(): kstep 32, bf16, pair_rows
}

// x: [n][H*W][x_cs] bf16 bits (cv1 reads channels [x_co, x_co + Cin)); w1 [c][Cin], b1 [c], w2 [Cout][4c], b2 [Cout] plain fp32;
// out: [n][H*W][out_cs] and cat: [n][H*W][cat_cs] bf16 bits, uploaded as the caller filled them (sentinels) and downloaded after the launch.
// *ok_out = sppf_fused_ok's verdict.  sppf_init runs once per process.  Returns the first HIP error code (launch_sppf_fused's
// hipErrorInvalidValue for what sppf_fused_ok refuses), or -1 without a launch for null pointers, non-positive sizes or buffers too small for the views.
extern "C" int sppf_probe_fused(const uint16_t* x, size_t x_elems, int x_cs, int x_co, int Cin,
                                const float* w1, const float* b1, int c, const float* w2, const float* b2, int Cout,
                                int n, int H, int W, int split, int dump,
                                uint16_t* out, size_t out_elems, int out_cs, int out_co,
                                uint16_t* cat, size_t cat_elems, int cat_cs, int* ok_out)
{
    if (!x || !w1 || !b1 || !w2 || !b2 || !out || !cat || !ok_out) return -1;
    if (n < 1 || n > 1024 || H < 1 || W < 1 || H > 4096 || W > 4096 || Cin < 1 || c < 1 || Cout < 1 || Cin > 4096 || c > 1024 || Cout > 4096) return -1;
    if (x_cs < 1 || out_cs < 1 || cat_cs < 1 || x_co < 0 || out_co < 0 || split < 1 || split > 64) return -1;
    if ((long)x_co + Cin > x_cs || (long)out_co + Cout > out_cs || 4L * c > cat_cs) return -1;
    const size_t px = (size_t)n * H * W;
    if (x_elems != px * x_cs || out_elems != px * out_cs || cat_elems != px * cat_cs) return -1;

    SppfArgs a{};
    a.x_cs = x_cs; a.x_co = x_co; a.Cin = Cin; a.out_cs = out_cs; a.out_co = out_co; a.Cout = Cout; a.cat_cs = cat_cs;
    a.H = H; a.W = W; a.n = n; a.c = c; a.split = split; a.dump = dump ? 1 : 0;
    *ok_out = sppf_fused_ok(a) ? 1 : 0;

    std::vector<uint8_t> w1p, w2p;
    std::vector<float> b1p, b2p;
    pack_1x1(w1, b1, c, Cin, &w1p, &b1p);
    pack_1x1(w2, b2, Cout, 4 * c, &w2p, &b2p);

    static bool inited = false;
    hipError_t rc = hipSuccess;
    if (!inited) { PROBE_TRY(sppf_init()); if (rc != hipSuccess) return (int)rc; inited = true; }
    unsigned char *d_x = nullptr, *d_out = nullptr, *d_cat = nullptr, *d_w1 = nullptr, *d_w2 = nullptr, *d_b1 = nullptr, *d_b2 = nullptr;
    hipStream_t s = nullptr;
    PROBE_TRY(hipMalloc((void**)&d_x, x_elems * 2));
    PROBE_TRY(hipMalloc((void**)&d_out, out_elems * 2));
    PROBE_TRY(hipMalloc((void**)&d_cat, cat_elems * 2));
    PROBE_TRY(hipMalloc((void**)&d_w1, w1p.size()));
    PROBE_TRY(hipMalloc((void**)&d_w2, w2p.size()));
    PROBE_TRY(hipMalloc((void**)&d_b1, b1p.size() * sizeof(float)));
    PROBE_TRY(hipMalloc((void**)&d_b2, b2p.size() * sizeof(float)));
    PROBE_TRY(hipStreamCreate(&s));
    if (rc == hipSuccess) {
        PROBE_TRY(hipMemcpyAsync(d_x, x, x_elems * 2, hipMemcpyHostToDevice, s));
        PROBE_TRY(hipMemcpyAsync(d_out, out, out_elems * 2, hipMemcpyHostToDevice, s));
        PROBE_TRY(hipMemcpyAsync(d_cat, cat, cat_elems * 2, hipMemcpyHostToDevice, s));
        PROBE_TRY(hipMemcpyAsync(d_w1, w1p.data(), w1p.size(), hipMemcpyHostToDevice, s));
        PROBE_TRY(hipMemcpyAsync(d_w2, w2p.data(), w2p.size(), hipMemcpyHostToDevice, s));
        PROBE_TRY(hipMemcpyAsync(d_b1, b1p.data(), b1p.size() * sizeof(float), hipMemcpyHostToDevice, s));
        PROBE_TRY(hipMemcpyAsync(d_b2, b2p.data(), b2p.size() * sizeof(float), hipMemcpyHostToDevice, s));
    }
    a.x = d_x; a.w1 = d_w1; a.b1 = (const float*)d_b1; a.w2 = d_w2; a.b2 = (const float*)d_b2; a.out = d_out; a.cat = d_cat;
    hipError_t launched = hipSuccess;
    if (rc == hipSuccess) launched = launch_sppf_fused(a, s);
    if (rc == hipSuccess) PROBE_TRY(hipStreamSynchronize(s));
    if (rc == hipSuccess) {
        PROBE_TRY(hipMemcpy(out, d_out, out_elems * 2, hipMemcpyDeviceToHost));
        PROBE_TRY(hipMemcpy(cat, d_cat, cat_elems * 2, hipMemcpyDeviceToHost));
    }
    if (s) PROBE_TRY(hipStreamDestroy(s));
    for (unsigned char* p : {d_x, d_out, d_cat, d_w1, d_w2, d_b1, d_b2})
        if (p) PROBE_TRY(hipFree(p));
    return (int)(rc != hipSuccess ? rc : launched);
}

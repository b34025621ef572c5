// head_bench.hip -- stand-alone timing of head_fused_kernel (the ablation of its predecessor is in profiles/r03_head_kernel_ablation.txt), and of its
// box_mode (the box branch's second conv inside the tail, at surviving waves): a sweep of the surviving-wave fraction by planted class logits, with
// s_memtime stamps around the conv phase (profiles/r06_head_bench_tail_box.txt).
// Originally: DIAGNOSTIC: what binds head_fused_kernel?  Runs the Detect tail of a YOLOv8n 416x416 batch (3549 anchors x n frames,
// random bf16 activations, class logits ~N(-2.75, 0.7) so that ~1.5 % of the anchors pass conf 0.5) with parts switched off:
//   bit 0: no weight-fragment loads (L1 / L2 traffic), bit 1: no activation loads (HBM), bit 2: stop after the class GEMM (no epilogue).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Izero-latency-yolo_amd/csrc -DZLY_HEAD_DIAG=1 zero-latency-yolo_amd/tools/head_bench.hip \
//         -o zero-latency-yolo_amd/_build/head_bench && ./zero-latency-yolo_amd/_build/head_bench
#include "../csrc/kernels_head.hip"
#include <stdio.h>
#include <string.h>
#include <random>
#include <vector>
using namespace zly;

static uint16_t f2bf(float f) { uint32_t u; memcpy(&u, &f, 4); return (uint16_t)((u + 0x7fff + ((u >> 16) & 1)) >> 16); }

struct Planted { std::vector<uint16_t> hc; std::vector<char> sign0; std::vector<float> bias20; void* box; void* stem; };

int main(int argc, char** argv)
{
    Planted planted[3];
    const int n = argc > 1 ? atoi(argv[1]) : 64;
    const int hw[3] = {2704, 676, 169}, Ws[3] = {52, 26, 13};
    std::mt19937 rng(3);
    std::normal_distribution<float> nd(0.f, 1.f);
    HeadArgs a; memset(&a, 0, sizeof a);
    int block0 = 0, off = 0;
    for (int l = 0; l < 3; ++l) {
        HeadLevel& L = a.lv[l];
        std::vector<uint16_t> hb((size_t)n * hw[l] * 64), hc((size_t)n * hw[l] * 80), wb(4 * 2 * 512), wc(5 * 3 * 512);
        for (auto& v : hb) v = f2bf(0.25f * nd(rng));
        for (auto& v : hc) v = f2bf(0.25f * nd(rng));
        for (auto& v : wb) v = f2bf(0.3f * nd(rng));
        for (auto& v : wc) v = f2bf(0.31f * nd(rng));            // logit std ~0.7 over 80 inputs of std 0.25
        std::vector<float> bb(64, 1.0f), bc(80, -2.75f);
        void *dhb, *dhc, *dwb, *dwc; float *dbb, *dbc;
        hipMalloc(&dhb, hb.size() * 2); hipMalloc(&dhc, hc.size() * 2); hipMalloc(&dwb, wb.size() * 2); hipMalloc(&dwc, wc.size() * 2);
        hipMalloc((void**)&dbb, 64 * 4); hipMalloc((void**)&dbc, 80 * 4);
        hipMemcpy(dhb, hb.data(), hb.size() * 2, hipMemcpyHostToDevice); hipMemcpy(dhc, hc.data(), hc.size() * 2, hipMemcpyHostToDevice);
        hipMemcpy(dwb, wb.data(), wb.size() * 2, hipMemcpyHostToDevice); hipMemcpy(dwc, wc.data(), wc.size() * 2, hipMemcpyHostToDevice);
        hipMemcpy(dbb, bb.data(), 64 * 4, hipMemcpyHostToDevice); hipMemcpy(dbc, bc.data(), 80 * 4, hipMemcpyHostToDevice);
        L.box_in = dhb; L.cls_in = dhc; L.box_cs = 64; L.cls_cs = 80; L.box_cin = 64; L.cls_cin = 80;
        L.wb = dwb; L.wc = dwc; L.bb = dbb; L.bc = dbc; L.nkb = 2; L.nkc = 3;
        // the tail's own box conv: the Detect stem buffer (160 channels per pixel, the box half first), cv2.L.1's weights as the dense op tiles them, its bias
        std::vector<uint16_t> hs((size_t)n * hw[l] * 160), w1(4 * 18 * 512);
        for (auto& v : hs) v = f2bf(0.25f * nd(rng));
        for (auto& v : w1) v = f2bf(0.05f * nd(rng));
        std::vector<float> b1(64, 0.1f);
        void *dhs, *dw1; float* db1;
        hipMalloc(&dhs, hs.size() * 2); hipMalloc(&dw1, w1.size() * 2); hipMalloc((void**)&db1, 64 * 4);
        hipMemcpy(dhs, hs.data(), hs.size() * 2, hipMemcpyHostToDevice); hipMemcpy(dw1, w1.data(), w1.size() * 2, hipMemcpyHostToDevice); hipMemcpy(db1, b1.data(), 64 * 4, hipMemcpyHostToDevice);
        L.w1 = dw1; L.b1 = db1; L.box2 = nullptr; L.box_mode = 0;
        planted[l].hc = hc; planted[l].box = dhb; planted[l].stem = dhs; planted[l].bias20.assign(80, -20.0f);
        planted[l].sign0.resize(80);
        for (int k = 0; k < 80; ++k) planted[l].sign0[(size_t)k] = (wc[(size_t)(((k / 32) * 64 + ((k % 32) / 8) * 16) * 8 + k % 8)] & 0x8000) ? 1 : 0;     // class 0's weight at k: tile 0, k-step k / 32, lane (k % 32 / 8) * 16 + 0
        L.H = Ws[l]; L.W = Ws[l]; L.hw = hw[l]; L.stride_px = 8 << l; L.anchor_off = off; L.block0 = block0; L.logits = nullptr; L.logits_cs = 144;
        block0 += (hw[l] + HEAD_GROUP - 1) / HEAD_GROUP; off += hw[l];
    }
    a.nc = 80; a.N_total = off; a.total_blocks = block0; a.only_level = -1; a.head = nullptr; a.conf_thr = 0.5f;
    FrameDesc* dd; std::vector<FrameDesc> hd((size_t)n); for (auto& d : hd) { d.src_off = 0; d.w = 416; d.h = 416; }
    hipMalloc((void**)&dd, n * sizeof(FrameDesc)); hipMemcpy(dd, hd.data(), n * sizeof(FrameDesc), hipMemcpyHostToDevice);
    a.desc = dd;
    hipMalloc((void**)&a.cand, (size_t)n * off * sizeof(Cand)); hipMalloc((void**)&a.cand_count, n * 4);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    const size_t nslots = (size_t)n * block0 * HEAD_WAVES;       // one cycle count per wave of the grid (zero: the wave did not run the conv)
    long nwaves = 0; for (int l = 0; l < 3; ++l) nwaves += (long)n * ((hw[l] + 15) / 16);
    unsigned long long* ddiag; hipMalloc((void**)&ddiag, nslots * 8);
    std::vector<unsigned long long> hdiag(nslots);
    hipMemcpyToSymbol(HIP_SYMBOL(g_head_diag), &ddiag, sizeof ddiag);
    // box 0: the tail as launched behind the dense cv2.L.1 (box_in = its output); box 1 / 2: the tail computes cv2.L.1 itself at surviving waves, from the
    // 160-channel Detect stem buffer, in conv3x3_ws_kernel's / conv3x3_lds_kernel's k-step order.  The class bias is -20 (nothing passes) and a fraction
    // `frac` of the 16-anchor waves gets ONE anchor whose class-0 logit is planted at about +20: the surviving-wave fraction is swept, not guessed.
    auto time_it = [&](const char* what, double frac) {
        float best = 1e9f, ms = 0;
        for (int rep = 0; rep < 30; ++rep) {
            hipMemsetAsync(a.cand_count, 0, n * 4, 0);
            hipMemsetAsync(ddiag, 0, nslots * 8, 0);
            hipEventRecord(e0, 0);
            if (launch_head_fused(ZLY_DTYPE_BF16, a, n, 0) != hipSuccess) { printf("launch failed\n"); exit(1); }
            hipEventRecord(e1, 0); hipEventSynchronize(e1);
            hipEventElapsedTime(&ms, e0, e1);
            if (ms < best) best = ms;
        }
        std::vector<int> cnt((size_t)n); hipMemcpy(cnt.data(), a.cand_count, n * 4, hipMemcpyDeviceToHost);
        hipMemcpy(hdiag.data(), ddiag, nslots * 8, hipMemcpyDeviceToHost);
        unsigned long long d[3] = {0, 0, (unsigned long long)nwaves};
        for (unsigned long long v : hdiag) if (v) { d[0] += v; d[1]++; }
        long tot = 0; for (int c : cnt) tot += c;
        printf("%-28s planted %.2f: %7.1f us   %.1f candidates per frame, %llu of %llu waves ran the conv (%.3f), %.0f cycles per conv phase\n", what, frac, best * 1e3,
               (double)tot / n, d[1], d[2], d[2] ? (double)d[1] / (double)d[2] : 0.0, d[1] ? (double)d[0] / (double)d[1] : 0.0);
    };
    time_it("random logits, dense input", -1.0);
    const double fracs[5] = {0.0, 0.1, 0.25, 0.5, 1.0};
    std::uniform_real_distribution<float> ud(0.f, 1.f);
    for (double frac : fracs) {
        for (int l = 0; l < 3; ++l) {
            HeadLevel& L = a.lv[l];
            const Planted& P = planted[l];
            std::vector<uint16_t> hc = P.hc;
            for (size_t t = 0; t < (size_t)n * ((hw[l] + 15) / 16); ++t) {
                if (!(ud(rng) < frac)) continue;
                const size_t f = t / ((hw[l] + 15) / 16), an = (t % ((hw[l] + 15) / 16)) * 16 + 3;
                if (an >= (size_t)hw[l]) continue;
                for (int k = 0; k < 80; ++k) hc[(f * hw[l] + an) * 80 + k] = P.sign0[(size_t)k] ? 0xc000 : 0x4000;      // -2 / +2: logit = 2 * sum |w0| - 20
            }
            hipMemcpy(const_cast<void*>(L.cls_in), hc.data(), hc.size() * 2, hipMemcpyHostToDevice);
            hipMemcpy(const_cast<float*>(L.bc), P.bias20.data(), 80 * 4, hipMemcpyHostToDevice);
        }
        for (int mode = 0; mode < 3; ++mode) {
            for (int l = 0; l < 3; ++l) {
                HeadLevel& L = a.lv[l];
                L.box_mode = mode; L.box_in = mode ? planted[l].stem : planted[l].box; L.box_cs = mode ? 160 : 64;
            }
            time_it(mode == 0 ? "dense input" : mode == 1 ? "tail conv, ws order" : "tail conv, lds order", frac);
        }
    }
    return 0;
}

// ws_pair_bench.hip -- DIAGNOSTIC build of conv3x3_ws_pair_kernel with s_memtime stamps around its phases (never part of libzly.so).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Izero-latency-yolo_amd/csrc -DZLY_WS_DIAG=1 zero-latency-yolo_amd/tools/ws_pair_bench.hip \
//         -o zero-latency-yolo_amd/_build/ws_pair_bench && ./zero-latency-yolo_amd/_build/ws_pair_bench
// Per shape: a chain of 20 bottlenecks back to back as the two conv3x3_ws_kernel launches each and as one pair launch each (us per bottleneck), and the
// pair kernel's per-wave cycle sums per tile: patch + conv A's weights + barrier | conv A | barrier + next-patch DMA issue | conv B (with the wait for
// conv B's weights) | wave total, against the bare MFMA cycles of the tile.
#include "../csrc/kernels_conv.hip"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
using namespace zly;

static void run(const char* name, int n, int H, int W, bool res)
{
    const int C = 64, nk = 18;
    std::vector<uint16_t> hin((size_t)n * H * W * C), hw((size_t)2 * C * nk * 32);
    for (size_t i = 0; i < hin.size(); ++i) hin[i] = 0x3c00 + (uint16_t)((i * 2654435761u >> 20) & 0x1ff);
    for (size_t i = 0; i < hw.size(); ++i) hw[i] = 0x3000 + (uint16_t)((i * 40503u >> 7) & 0x3ff) ^ ((i & 1) << 15);
    void *din, *dw, *dmid, *dout; float* dbias; unsigned long long* ddbg;
    hipMalloc(&din, hin.size() * 2); hipMalloc(&dw, hw.size() * 2); hipMalloc(&dmid, hin.size() * 2); hipMalloc(&dout, hin.size() * 2);
    hipMalloc((void**)&dbias, C * 4); hipMemset(dbias, 0, C * 4);
    hipMemcpy(din, hin.data(), hin.size() * 2, hipMemcpyHostToDevice); hipMemcpy(dw, hw.data(), hw.size() * 2, hipMemcpyHostToDevice);
    ConvArgs a; memset(&a, 0, sizeof a);
    a.in = din; a.in_cs = C; a.H = H; a.W = W; a.Cin = C; a.wgt = dw; a.bias = dbias;
    a.out = dmid; a.out_cs = C; a.Ho = H; a.Wo = W; a.Cout = C; a.cout_pad = C; a.stride = 1; a.pad = 1;
    a.K = 9 * C; a.nk = nk; a.M = n * H * W; a.act = 1;
    ConvArgs b = a;
    b.in = dmid; b.out = dout; b.wgt = (const char*)dw + (size_t)C * nk * 64;
    if (res) { b.res = din; b.res_cs = C; }
    conv_init();
    Switches sw;
    sw.ws_pair_max_tiles = 1 << 20;                               // every size: this tool is what the planner's gate is set with
    if (const char* v = getenv("ZLY_WS_PAIR_GRID")) sw.ws_pair_grid = atoi(v);      // e.g. 256: one workgroup per CU, two tiles each
    ConvPlan pa{}, pb{};
    WsPairPlan pp{};
    if (!plan_ws(a, sw, &pa) || !plan_ws(b, sw, &pb) || !conv_ws_pair_plan(a, b, pa, pb, sw, &pp)) { printf("%s: no plan\n", name); return; }
    const size_t nw = (size_t)pp.gx * 4;
    hipMalloc((void**)&ddbg, nw * 64); hipMemset(ddbg, 0, nw * 64);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    const int CHAIN = 20;
    float ms = 0, best2 = 1e9f, best1 = 1e9f;
    unsigned long long* none = nullptr;
    hipMemcpyToSymbol(HIP_SYMBOL(g_ws_diag), &none, sizeof none);
    for (int rep = 0; rep < 12; ++rep) {
        hipEventRecord(e0, 0);
        for (int k = 0; k < CHAIN; ++k) { launch_conv(a, pa, 0); launch_conv(b, pb, 0); }
        hipEventRecord(e1, 0); hipEventSynchronize(e1);
        hipEventElapsedTime(&ms, e0, e1);
        if (rep >= 2 && ms < best2) best2 = ms;
    }
    hipMemcpyToSymbol(HIP_SYMBOL(g_ws_diag), &ddbg, sizeof ddbg);
    for (int rep = 0; rep < 12; ++rep) {
        hipEventRecord(e0, 0);
        for (int k = 0; k < CHAIN; ++k) launch_conv_ws_pair(a, b, pp, false, 0);
        hipEventRecord(e1, 0); hipEventSynchronize(e1);
        hipEventElapsedTime(&ms, e0, e1);
        if (rep >= 2 && ms < best1) best1 = ms;
    }
    std::vector<unsigned long long> h(nw * 8);
    hipMemcpy(h.data(), ddbg, nw * 64, hipMemcpyDeviceToHost);
    double s[5] = {0}; for (size_t w = 0; w < nw; ++w) for (int k = 0; k < 5; ++k) s[k] += (double)h[w * 8 + k];
    const double tpw = (double)pp.g.total_tiles / pp.gx;
    const int nct = (pp.g.TH * pp.g.TW + 15) / 16;
    printf("%-26s tile %dx%d lds=%uKB grid %u (%.2f tiles each): two launches %.2f us, pair %.2f us per bottleneck (chain of %d, best of 10) | cycles/tile/wave: patch + wA + barrier %.0f  conv A %.0f  barrier + dma issue %.0f  conv B %.0f | wave total %.0f (bare MFMA %d)\n",
           name, pp.g.TH, pp.g.TW, pp.lds / 1024, pp.gx, tpw, best2 * 1e3 / CHAIN, best1 * 1e3 / CHAIN, CHAIN,
           s[0] / nw / tpw, s[1] / nw / tpw, s[2] / nw / tpw, s[3] / nw / tpw, s[4] / nw / tpw, ((pp.g.TH + 3) / 2 * 2 + nct) * nk * 16);
    hipFree(din); hipFree(dw); hipFree(dmid); hipFree(dout); hipFree(dbias); hipFree(ddbg);
}

int main()
{
    run("26x26 x64", 64, 26, 26, false);
    run("26x26 x64 shortcut", 64, 26, 26, true);
    run("26x26 x16", 16, 26, 26, false);
    run("40x40 x32", 32, 40, 40, true);
    run("40x40 x48", 48, 40, 40, true);
    run("40x40 x64", 64, 40, 40, true);
    run("80x80 x8", 8, 80, 80, true);
    run("80x80 x12", 12, 80, 80, true);
    run("80x80 x16", 16, 80, 80, true);
    run("80x80 x32", 32, 80, 80, true);
    run("80x80 x32 no shortcut", 32, 80, 80, false);
    return 0;
}

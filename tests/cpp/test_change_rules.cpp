// The change map's rules on the CPU (csrc/change_device.h through the host twin of csrc/change_rules.h), for tests/test_change_rules.py: no GPU, nothing
// of the engine.  The program reads a script from stdin and keeps up to 16 streams:
//   cfg <cell> <threshold_q4> <max_active_permille> <max_peaks> <window_w> <window_h>
//   reset <stream>                                      (-1: every stream)
//   plan <K> {<x0> <y0> <w> <h> <slot> <track_id>} x K  the plan of the NEXT frame: its track regions are the initial suppression, and it is filled
//   frame <stream> <fmt> <w> <h> <off0> <off1> <off2> <pitch0> <pitch1> <pitch2> <file>
//       the view of the buffer in <file>; checked as the engine checks it (chip_check_view, change_check_size).  Prints
//       refused <code>
//     or
//       hdr <n_cells> <n_active> <n_peaks> <flags> <gw> <gh> <step> <pad> outside <needed bytes of the sums pass outside their plane's extent>
//       sums <S...>
//       act <A...>
//       peak <x0> <y0> <w> <h> <cx> <cy> <activity> <pad>      per peak
//       plan {<x0> <y0> <w> <h> <slot> <track_id>} x K         if a plan was given
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "change_rules.h"

using namespace zly;

int main()
{
    zly_change_config cfg;
    change_default_config(416, 416, &cfg);
    std::vector<ChangeStateHost> streams(16);
    std::vector<zly_zoom_region> plan;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        if (!(in >> op) || op[0] == '#') continue;
        if (op == "cfg") {
            in >> cfg.cell >> cfg.threshold_q4 >> cfg.max_active_permille >> cfg.max_peaks >> cfg.window_w >> cfg.window_h;
            std::string err;
            if (int rc = change_check_config(&cfg, 16, &err)) { std::printf("refused %d\n", rc); return 2; }
        } else if (op == "reset") {
            int s = 0;
            in >> s;
            for (int i = 0; i < 16; ++i) if (s < 0 || s == i) streams[(size_t)i].st = ChangeStream{};
        } else if (op == "plan") {
            int K = 0;
            in >> K;
            plan.assign((size_t)K, zly_zoom_region{});
            for (auto& r : plan) in >> r.x0 >> r.y0 >> r.w >> r.h >> r.slot >> r.track_id;
        } else if (op == "frame") {
            int s = 0;
            zly_frame_view v{};
            std::string path;
            in >> s >> v.fmt >> v.w >> v.h >> v.off[0] >> v.off[1] >> v.off[2] >> v.pitch[0] >> v.pitch[1] >> v.pitch[2] >> path;
            std::ifstream file(path, std::ios::binary);
            const std::vector<char> bytes((std::istreambuf_iterator<char>(file)), std::istreambuf_iterator<char>());
            // an exact-size copy: the sanitizer build sees a read one byte behind the buffer
            std::vector<uint8_t> buf(bytes.begin(), bytes.end());
            std::string err;
            int rc = chip_check_view(0, buf.data(), buf.size(), &v, &err);
            if (!rc) rc = change_check_size(v.w, v.h, cfg.cell, &err);
            if (rc || s < 0 || s >= 16) { std::printf("refused %d\n", rc ? rc : (int)ZLY_ERR_INVALID_ARGUMENT); continue; }
            const ChipFrame f = chip_frame_of(&v);
            const int nc = change_cells_axis(v.w, cfg.cell) * change_cells_axis(v.h, cfg.cell);
            std::vector<uint32_t> S((size_t)nc), act((size_t)nc);
            uint64_t outside = 0;
            change_sums_host(buf.data(), f, cfg.cell, S.data(), &outside);
            zly_change_header hd;
            zly_change_peak peaks[ZLY_CHANGE_MAX_PEAKS];
            change_pick_host(streams[(size_t)s], S.data(), v.w, v.h, cfg, plan.data(), (int)plan.size(), &hd, peaks, act.data());
            std::printf("hdr %d %d %d %u %d %d %u %u outside %llu\n", hd.n_cells, hd.n_active, hd.n_peaks, hd.flags, hd.gw, hd.gh, hd.step, hd.pad,
                        (unsigned long long)outside);
            std::printf("sums");
            for (uint32_t x : S) std::printf(" %u", x);
            std::printf("\nact");
            for (uint32_t x : act) std::printf(" %u", x);
            std::printf("\n");
            for (int p = 0; p < hd.n_peaks; ++p)
                std::printf("peak %d %d %d %d %d %d %u %u\n", peaks[p].x0, peaks[p].y0, peaks[p].w, peaks[p].h, peaks[p].cx, peaks[p].cy, peaks[p].activity, peaks[p].pad);
            if (!plan.empty()) {
                change_fill_host(plan.data(), (int)plan.size(), peaks, hd.n_peaks);
                std::printf("plan");
                for (const auto& r : plan) std::printf(" %d %d %d %d %d %u", r.x0, r.y0, r.w, r.h, r.slot, r.track_id);
                std::printf("\n");
                plan.clear();
            }
        } else {
            std::fprintf(stderr, "unknown op %s\n", op.c_str());
            return 2;
        }
    }
    return 0;
}

// The camera motion's rules on the CPU (csrc/camera_device.h through the host twin of csrc/camera_rules.h), for tests/test_camera_rules.py: no GPU,
// nothing of the engine.  The program reads a script from stdin and keeps up to 16 streams, each with a track table of 64 slots:
//   cfg <cell> <radius> <max_residual_q4>
//   reset <stream>                                      (-1: every stream)
//   frame <stream> <fmt> <w> <h> <off0> <off1> <off2> <pitch0> <pitch1> <pitch2> <file>
//       the view of the buffer in <file>; checked as the engine checks it (chip_check_view, camera_check_size).  Prints
//       refused <code>
//     or the stream's whole record:
//       hdr <flags> <step> <gw> <gh> <dx> <dy> <fx> <fy> <sx_q4> <sy_q4> <n_lost> <n_applied> <sad_min> <sad_zero> <pend_x_q4> <pend_y_q4> <pad x 4>
//       sad <the 289 entries of the table, untouched ones included>
//   tracks <stream> <T> {<live> <x bits> <y bits>} x T    the stream's slots 0 .. T-1 (x, y as the u32 patterns of their fp32 values); the others are free
//   apply <stream>                                        step A.  Prints
//       xy {<x bits> <y bits>} x 64
//     and the record as above
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "camera_rules.h"

using namespace zly;

struct Slots { uint32_t live[64] = {}; float x[64] = {}, y[64] = {}; };

static void print_record(CameraStateHost& s)
{
    const zly_camera_header h = s.header();
    std::printf("hdr %u %u %d %d %d %d %d %d %d %d %u %u %llu %llu %lld %lld %u %u %u %u\n", h.flags, h.step, h.gw, h.gh, h.dx, h.dy, h.fx, h.fy, h.sx_q4, h.sy_q4,
                h.n_lost, h.n_applied, (unsigned long long)h.sad_min, (unsigned long long)h.sad_zero, (long long)h.pend_x_q4, (long long)h.pend_y_q4,
                h.pad[0], h.pad[1], h.pad[2], h.pad[3]);
    std::printf("sad");
    const uint64_t* tab = s.table();
    for (uint64_t i = 0; i < camera_layout().sad_room; ++i) std::printf(" %llu", (unsigned long long)tab[i]);
    std::printf("\n");
}

int main()
{
    zly_camera_config cfg;
    camera_default_config(&cfg);
    std::vector<CameraStateHost> streams(16);
    std::vector<Slots> tables(16);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        if (!(in >> op) || op[0] == '#') continue;
        if (op == "cfg") {
            in >> cfg.cell >> cfg.radius >> cfg.max_residual_q4;
            std::string err;
            if (int rc = camera_check_config(&cfg, 16, &err)) { std::printf("refused %d\n", rc); return 2; }
        } else if (op == "reset") {
            int s = 0;
            in >> s;
            for (int i = 0; i < 16; ++i) if (s < 0 || s == i) camera_reset_host(streams[(size_t)i]);
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
            if (!rc) rc = camera_check_size(v.w, v.h, cfg.cell, cfg.radius, &err);
            if (rc || s < 0 || s >= 16) { std::printf("refused %d\n", rc ? rc : (int)ZLY_ERR_INVALID_ARGUMENT); continue; }
            const ChipFrame f = chip_frame_of(&v);
            const int nc = change_cells_axis(v.w, cfg.cell) * change_cells_axis(v.h, cfg.cell);
            std::vector<uint32_t> S((size_t)nc);
            change_sums_host(buf.data(), f, cfg.cell, S.data(), nullptr);
            camera_frame_host(streams[(size_t)s], S.data(), v.w, v.h, cfg);
            print_record(streams[(size_t)s]);
        } else if (op == "tracks") {
            int s = 0, T = 0;
            in >> s >> T;
            if (s < 0 || s >= 16 || T < 0 || T > 64) { std::fprintf(stderr, "bad tracks line\n"); return 2; }
            Slots& tb = tables[(size_t)s];
            tb = Slots{};
            for (int t = 0; t < T; ++t) {
                uint32_t xb = 0, yb = 0;
                in >> tb.live[t] >> xb >> yb;
                std::memcpy(&tb.x[t], &xb, 4); std::memcpy(&tb.y[t], &yb, 4);
            }
        } else if (op == "apply") {
            int s = 0;
            in >> s;
            if (s < 0 || s >= 16) { std::fprintf(stderr, "bad apply line\n"); return 2; }
            Slots& tb = tables[(size_t)s];
            camera_apply_host(streams[(size_t)s], tb.x, tb.y, tb.live, 64);
            std::printf("xy");
            for (int t = 0; t < 64; ++t) {
                uint32_t xb = 0, yb = 0;
                std::memcpy(&xb, &tb.x[t], 4); std::memcpy(&yb, &tb.y[t], 4);
                std::printf(" %u %u", xb, yb);
            }
            std::printf("\n");
            print_record(streams[(size_t)s]);
        } else {
            std::fprintf(stderr, "unknown op %s\n", op.c_str());
            return 2;
        }
    }
    return 0;
}

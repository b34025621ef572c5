// test_chip_rules.cpp -- the chips' rules as the product's own text computes them on a CPU (tests/test_chip_rules.py drives it): csrc/chip_device.h --
// the rectangle, the selection predicate, the slab offsets and the per-format sample addresses the kernels execute -- and the host checks of
// csrc/chip_rules.h over csrc/frame_rules.h.  No GPU, nothing of the engine.
//
//   test_chip_rules run < script      one case per line:
//       case BUF_FILE FLAGS FMT W H OFF0 OFF1 OFF2 PITCH0 PITCH1 PITCH2  SLAB_FILE CAP  CHIP_W CHIP_H MAX_CHIPS CLASS_ID SCALE_BITS LAYOUT
//     BUF_FILE holds the caller's whole buffer, SLAB_FILE one slab of capacity CAP; FLAGS are the engine's (zly_config.flags); SCALE_BITS the
//     fp32 scale in hex.  Printed per case: "refused RC" if the config or the view is refused; otherwise
//       hdr N_CHIPS N_ELIGIBLE FRAME_TAG FLAGS / rec DET CLASS TRACK CONF_BITS X0 Y0 W H (N_CHIPS times) / chip HEX (N_CHIPS times: the chip's bytes
//       in the config's layout) / violations N
//     A chip is cut pixel by pixel: every source pixel's samples are fetched at chip_pixel_samples' addresses and converted by include/zly.h's
//     formulas, and the filter is area_device.h's.  A sample address, or a byte of chip_row_bytes' ranges as the cut kernel stages them, that lies
//     outside its plane's extent counts as a violation (and is not read).
//       call N MAX_BATCH FRAMES DSLABS SOURCE      -> "rc RC" of chip_check_call (FRAMES, DSLABS: 0 = null)
//       layout CHIP_W CHIP_H MAX_CHIPS LAYOUT      -> "layout SLAB_BYTES PIXELS_OFF CHIP_STRIDE CHIP_BYTES"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "chip_rules.h"
#include "area_device.h"

using namespace zly;

static std::vector<uint8_t> read_file(const std::string& path)
{
    std::vector<uint8_t> v;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path.c_str()); exit(2); }
    uint8_t tmp[65536];
    size_t n;
    while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) v.insert(v.end(), tmp, tmp + n);
    fclose(f);
    return v;
}

static long g_violations = 0;

// is [o, o + n) inside plane p of the frame?
static bool inside(const ChipFrame& f, int p, uint64_t o, uint64_t n) { return o >= f.off[p] && o + n <= f.off[p] + f.ext[p]; }

// include/zly.h: Y, U, V -> B, G, R in int32, >> arithmetic
static void yuv_to_bgr(int Y, int U, int V, bool b709, int out[3])
{
    const int CY = b709 ? 1220945 : 1220542, CVR = b709 ? 1879825 : 1673527, CVG = b709 ? -558796 : -852492;
    const int CUG = b709 ? -223607 : -409993, CUB = b709 ? 2215014 : 2116026;
    const int yy = (Y - 16 > 0 ? Y - 16 : 0) * CY, u = U - 128, v = V - 128;
    auto cl = [](int x) { return x < 0 ? 0 : x > 255 ? 255 : x; };
    out[2] = cl((yy + CVR * v + (1 << 19)) >> 20);
    out[1] = cl((yy + CVG * v + CUG * u + (1 << 19)) >> 20);
    out[0] = cl((yy + CUB * u + (1 << 19)) >> 20);
}

// frame pixel (x, y) as B, G, R through the header's addressing; false (and a violation) if a sample lies outside its plane
static bool pixel_bgr(const std::vector<uint8_t>& buf, const ChipFrame& f, int x, int y, int bgr[3])
{
    uint64_t o[3];
    int32_t nb[3], pl[3];
    const int k = chip_pixel_samples(f, x, y, o, nb, pl);
    for (int i = 0; i < k; ++i)
        if (!inside(f, pl[i], o[i], (uint64_t)nb[i]) || o[i] + (uint64_t)nb[i] > buf.size()) { ++g_violations; return false; }
    const int fmt = f.fmt;
    if (f.fam == ZLY_CHIP_FAM_PACKED) {
        const uint8_t* q = &buf[o[0]];
        const bool rgb = fmt == ZLY_PIX_RGB || fmt == ZLY_PIX_RGBA;
        bgr[0] = rgb ? q[2] : q[0]; bgr[1] = q[1]; bgr[2] = rgb ? q[0] : q[2];
        return true;
    }
    if (f.fam == ZLY_CHIP_FAM_Y422) {
        const uint8_t* m = &buf[o[0]];
        const bool uyvy = fmt == ZLY_PIX_UYVY_BT601 || fmt == ZLY_PIX_UYVY_BT709;
        const int Y = uyvy ? m[1 + (x & 1) * 2] : m[(x & 1) * 2], U = uyvy ? m[0] : m[1], V = uyvy ? m[2] : m[3];
        yuv_to_bgr(Y, U, V, fmt >= ZLY_PIX_YUY2_BT709, bgr);
        return true;
    }
    const bool b709 = fmt == ZLY_PIX_NV12_BT709 || fmt == ZLY_PIX_I420_BT709;
    if (f.fam == ZLY_CHIP_FAM_NV12) yuv_to_bgr(buf[o[0]], buf[o[1]], buf[o[1] + 1], b709, bgr);
    else yuv_to_bgr(buf[o[0]], buf[o[1]], buf[o[2]], b709, bgr);
    return true;
}

// the byte ranges the cut kernel stages for the rectangle: chunks of ZLY_CHIP_CHUNK_PX frame columns from x0 & ~1 on, every row, every plane
static void check_row_ranges(const ChipFrame& f, const zly_chip_rec& r)
{
    const int xs0 = r.x0 & ~1, xs1 = r.x0 + r.w;
    for (int y = r.y0; y < r.y0 + r.h; ++y)
        for (int xa = xs0; xa < xs1; xa += ZLY_CHIP_CHUNK_PX) {
            const int xb = xa + ZLY_CHIP_CHUNK_PX < xs1 ? xa + ZLY_CHIP_CHUNK_PX : xs1;
            for (int p = 0; p < f.planes; ++p) {
                uint32_t nb = 0;
                const uint64_t o = chip_row_bytes(f, p, y, xa, xb, &nb);
                if (!inside(f, p, o, nb)) ++g_violations;
                if ((uint64_t)nb + 15u >= (uint64_t)ZLY_CHIP_THREADS * 16u) ++g_violations;      // one 16-byte lane load per thread, alignment slack included
            }
        }
}

static void cut_chip(const std::vector<uint8_t>& buf, const ChipFrame& f, const zly_chip_rec& r, const zly_chip_config& c, std::vector<uint8_t>* out)
{
    const int Dx = c.chip_w, Dy = c.chip_h, Sx = r.w, Sy = r.h;
    const int64_t T = (int64_t)Sx * Sy;
    const bool f32 = c.layout == ZLY_CHIP_RGB_F32;
    out->assign((size_t)Dx * Dy * (f32 ? 12 : 3), 0);
    for (int dy = 0; dy < Dy; ++dy) {
        const AreaSpan sy = area_span(Sy, Dy, dy);
        for (int dx = 0; dx < Dx; ++dx) {
            const AreaSpan sx = area_span(Sx, Dx, dx);
            int64_t acc[3] = {0, 0, 0};
            for (int iy = sy.i0; iy <= sy.i1; ++iy) {
                int64_t hs[3] = {0, 0, 0};
                for (int ix = sx.i0; ix <= sx.i1; ++ix) {
                    int p[3] = {0, 0, 0};
                    if (!pixel_bgr(buf, f, r.x0 + ix, r.y0 + iy, p)) continue;
                    const int w = area_weight(sx, Dx, ix);
                    for (int k = 0; k < 3; ++k) hs[k] += (int64_t)w * p[k];
                }
                const int wy = area_weight(sy, Dy, iy);
                for (int k = 0; k < 3; ++k) acc[k] += (int64_t)wy * hs[k];
            }
            for (int k = 0; k < 3; ++k) {
                const int v = (int)((acc[k] + (T >> 1)) / T);
                if (f32) {
                    const float q = (float)v / 255.0f;
                    memcpy(&(*out)[(((size_t)(2 - k) * Dy + dy) * Dx + dx) * 4], &q, 4);
                } else (*out)[((size_t)dy * Dx + dx) * 3 + k] = (uint8_t)v;
            }
        }
    }
}

static int run_case(std::istringstream& in)
{
    std::string buf_file, slab_file;
    int32_t flags = 0, cap = 0;
    zly_frame_view v{};
    zly_chip_config c{};
    uint32_t scale_bits = 0;
    in >> buf_file >> flags >> v.fmt >> v.w >> v.h >> v.off[0] >> v.off[1] >> v.off[2] >> v.pitch[0] >> v.pitch[1] >> v.pitch[2] >> slab_file >> cap >>
        c.chip_w >> c.chip_h >> c.max_chips >> c.class_id >> std::hex >> scale_bits >> std::dec >> c.layout;
    if (!in) { fprintf(stderr, "bad case line\n"); return 2; }
    memcpy(&c.scale, &scale_bits, 4);
    const std::vector<uint8_t> buf = read_file(buf_file), slab = read_file(slab_file);
    std::string err;
    if (int rc = chip_check_config(&c, cap, &err)) { printf("refused %d\n", rc); return 0; }
    if (int rc = chip_check_view(flags, buf.data(), buf.size(), &v, &err)) { printf("refused %d\n", rc); return 0; }
    if (slab.size() != sizeof(zly_slab_header) + (size_t)cap * sizeof(zly_det)) { fprintf(stderr, "slab file of the wrong size\n"); return 2; }
    const ChipFrame f = chip_frame_of(&v);
    zly_slab_header sh;
    memcpy(&sh, slab.data(), sizeof sh);
    const int K = chip_stored(sh.n_kept, cap);
    std::vector<zly_chip_rec> recs;
    int n_elig = 0;
    for (int d = 0; d < K; ++d) {
        zly_det D;
        memcpy(&D, slab.data() + sizeof sh + (size_t)d * sizeof D, sizeof D);
        if (!chip_eligible(D.class_id, c.class_id)) continue;
        if (n_elig++ >= c.max_chips) continue;
        const ChipSpan sx = chip_rect_axis(D.x, D.w, c.scale, f.W), sy = chip_rect_axis(D.y, D.h, c.scale, f.H);
        zly_chip_rec r;
        r.det = d; r.class_id = D.class_id; r.track_id = D.track_id; r.confidence = D.confidence;
        r.x0 = sx.o; r.y0 = sy.o; r.w = sx.n; r.h = sy.n;
        recs.push_back(r);
    }
    g_violations = 0;
    printf("hdr %d %d %u %u\n", (int)recs.size(), n_elig, sh.frame_tag, 0u);
    for (const zly_chip_rec& r : recs) {
        uint32_t cb;
        memcpy(&cb, &r.confidence, 4);
        printf("rec %d %d %u %x %d %d %d %d\n", r.det, r.class_id, r.track_id, cb, r.x0, r.y0, r.w, r.h);
    }
    std::vector<uint8_t> chip;
    for (const zly_chip_rec& r : recs) {
        if (r.x0 < 0 || r.y0 < 0 || r.w < 1 || r.h < 1 || r.x0 + r.w > f.W || r.y0 + r.h > f.H) { ++g_violations; printf("chip\n"); continue; }
        check_row_ranges(f, r);
        cut_chip(buf, f, r, c, &chip);
        fputs("chip ", stdout);
        for (uint8_t b : chip) printf("%02x", b);
        fputc('\n', stdout);
    }
    printf("violations %ld\n", g_violations);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2 || strcmp(argv[1], "run") != 0) { fprintf(stderr, "usage: test_chip_rules run < script\n"); return 2; }
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string verb;
        if (!(in >> verb)) continue;
        if (verb == "case") {
            if (int rc = run_case(in)) return rc;
        } else if (verb == "call") {
            int n = 0, max_batch = 0, frames = 0, dslabs = 0, source = 0;
            in >> n >> max_batch >> frames >> dslabs >> source;
            std::string err;
            static const int dummy = 0;
            printf("rc %d\n", chip_check_call(n, max_batch, frames ? &dummy : nullptr, dslabs ? &dummy : nullptr, source, &err));
        } else if (verb == "layout") {
            int w = 0, h = 0, m = 0, l = 0;
            in >> w >> h >> m >> l;
            const ChipLayout y = chip_layout(w, h, m, l == ZLY_CHIP_RGB_F32);
            printf("layout %llu %llu %llu %llu\n", (unsigned long long)y.slab_bytes, (unsigned long long)y.pixels_off, (unsigned long long)y.chip_stride,
                   (unsigned long long)y.chip_bytes);
        } else { fprintf(stderr, "unknown verb %s\n", verb.c_str()); return 2; }
    }
    return 0;
}

// kernels_chips.hip -- the chips (include/zly.h "Chips"; the arithmetic: chip_device.h) on gfx950: a fixed-size, area-resized crop of the frame for each
// of a slab's detections, cut where slab and frame lie in HBM.
//
// chip_select_kernel: one workgroup of ONE wavefront per frame, in the manner of zoom_plan_kernel.  It walks the slab's K stored detections 64 at a
//   time; a ballot of the eligible lanes and the popcount of the lanes below give every eligible detection its chip slot, and the lanes whose slot is
//   below max_chips store their record (the rectangle of step 4: chip_rect_axis).  Lane 0 stores the header last.
// chip_cut_kernel: grid = (band of ZLY_CHIP_BAND_ROWS chip rows) x (chip slot j) x (frame).  A workgroup whose j >= n_chips -- read from the header
//   the select kernel has just written, in stream order -- leaves at once.  One thread per chip column.  The scheme is area_kernel's (kernels_area.hip),
//   with the footprints taken inside the record's rectangle and every staged row addressed in FRAME coordinates:
//   Loads.   A workgroup walks the frame rows its band's footprints cover.  Each row of the rectangle -- ZLY_CHIP_CHUNK_PX frame pixels of it at a
//            time, from the even column x0 & ~1 on, so that a pixel's chroma sample is staged with it whatever the parity of x0 -- is staged into
//            LDS, plane by plane, with one 16-byte load per lane on consecutive 16-byte-aligned addresses.  Only a lane whose 16 bytes would leave
//            the plane's extent loads byte by byte, inside it.
//   Double buffering.  The next unit's loads are issued into registers before the current unit is consumed from LDS; one barrier per unit.
//   Accumulation.  Horizontal footprint sums from LDS into three int32 (converting the format on the way: yuv_device.h), wy * hsum into 64-bit
//            accumulators, one exact division per output byte.  A rectangle smaller than the chip takes the same path: several chip columns and rows
//            then share a source pixel.
// The format is uniform per workgroup.  Stores are per-lane vector stores in plain C++.  FP contraction is OFF for this file and the pragma stands in
// front of chip_device.h, which holds the float arithmetic of the rectangle (its functions also turn it off in their own bodies).
#include "zly_internal.h"
#include "yuv_device.h"
#include "area_device.h"

#pragma clang fp contract(off)

#include "chip_device.h"

namespace zly {

static_assert(sizeof(zly_chip_header) == ZLY_CHIP_HDR_BYTES && sizeof(zly_chip_rec) == ZLY_CHIP_REC_BYTES && sizeof(zly_det) == 40, "record sizes");

// ---- selection --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void chip_select_kernel(const uint8_t* __restrict__ slabs, unsigned long long slab_bytes, int cap,
                                                         const ChipFrame* __restrict__ frames, uint8_t* __restrict__ chips, unsigned long long chip_slab_bytes,
                                                         int max_chips, int class_id, float scale)
{
    const int lane = threadIdx.x;
    const int f = blockIdx.x;
    const uint8_t* slab = slabs + (size_t)f * slab_bytes;
    const zly_slab_header sh = *reinterpret_cast<const zly_slab_header*>(slab);
    const zly_det* dets = reinterpret_cast<const zly_det*>(slab + sizeof(zly_slab_header));
    uint8_t* out = chips + (size_t)f * chip_slab_bytes;
    const int W = frames[f].W, H = frames[f].H;
    const int K = chip_stored(sh.n_kept, cap);
    int count = 0;                                                          // eligible detections in front of this round
    for (int base = 0; base < K; base += 64) {
        const int d = base + lane;
        zly_det D = {};
        if (d < K) D = dets[d];
        const bool elig = d < K && chip_eligible(D.class_id, class_id);
        const unsigned long long E = __ballot(elig);
        const int slot = count + __popcll(E & ((1ull << lane) - 1ull));
        if (elig && slot < max_chips) {
            const ChipSpan sx = chip_rect_axis(D.x, D.w, scale, W), sy = chip_rect_axis(D.y, D.h, scale, H);
            zly_chip_rec r;
            r.det = d; r.class_id = D.class_id; r.track_id = D.track_id; r.confidence = D.confidence;
            r.x0 = sx.o; r.y0 = sy.o; r.w = sx.n; r.h = sy.n;
            *reinterpret_cast<zly_chip_rec*>(out + chip_rec_off(slot)) = r;
        }
        count += __popcll(E);
    }
    if (lane == 0) {
        zly_chip_header h;
        h.n_chips = count < max_chips ? count : max_chips; h.n_eligible = count; h.frame_tag = sh.frame_tag; h.flags = 0u;
        *reinterpret_cast<zly_chip_header*>(out) = h;
    }
}

// ---- the cut ----------------------------------------------------------------------------------------------------------------------------
typedef unsigned int chip_u32x4 __attribute__((ext_vector_type(4)));

#define CHIP_PLANE_LDS 4096                  // LDS bytes per plane and buffer: 256 lanes x 16 bytes
static_assert(ZLY_CHIP_CHUNK_PX % 2 == 0, "a staging chunk starts at an even frame column (4:2:0 and 4:2:2 chroma)");
static_assert(ZLY_CHIP_CHUNK_PX * 4 + 15 < CHIP_PLANE_LDS, "a chunk of the widest format plus its alignment slack fits one lane load per thread");
static_assert(CHIP_PLANE_LDS == ZLY_CHIP_THREADS * 16, "one 16-byte load per lane and plane");
static_assert(ZLY_CHIP_MAX_DIM <= ZLY_CHIP_THREADS, "one thread per chip column");

// lane t's 16 bytes at q: the aligned vector load where all of it lies inside [lo, hi), single bytes of the plane otherwise
__device__ __forceinline__ chip_u32x4 chip_load16(const uint8_t* q, const uint8_t* lo, const uint8_t* hi)
{
    if (q >= lo && q + 16 <= hi) return *reinterpret_cast<const chip_u32x4*>(q);
    chip_u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        unsigned int x = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint8_t* c = q + k * 4 + b;
            if (c >= lo && c < hi) x |= (unsigned int)*c << (8 * b);
        }
        v[k] = x;
    }
    return v;
}

// (acc + T/2) / T for acc <= 255 * T, T <= 2^28: exact
__device__ __forceinline__ unsigned int chip_round_div(unsigned long long acc, unsigned int T, float inv_t)
{
    const unsigned long long num = acc + (T >> 1);
    unsigned int q = (unsigned int)((float)num * inv_t);            // the quotient is at most 255 and the estimate's relative error below 2^-21: within one
    const long long r = (long long)num - (long long)((unsigned long long)q * T);
    if (r < 0) --q; else if (r >= (long long)T) ++q;
    return q;
}

enum { CHIP_PACKED = 0, CHIP_PACKED32 = 1, CHIP_YUV420 = 2, CHIP_YUV422 = 3 };      // PACKED32: 4-byte pixels at 4-byte-aligned LDS offsets, one dword read each

// t0, t1, t2 += the weighted sums over FRAME columns [ia, ib] of a staged row (its unit begins at the even frame column xa; [ia, ib] lies inside the
// unit and inside x0 + sx, the footprint of the thread's chip column).  The values are B, G, R for the YUV families and bytes 0, 1, 2 of the pixel for
// the packed ones.  rel = i - xa has the frame column's parity, so a pixel's chroma sample is its own.
template <int FAM>
__device__ __forceinline__ void chip_row_sums(const uint8_t* L0, const uint8_t* L1, const uint8_t* L2, int fmt, unsigned int bpp, bool nv12, const AreaSpan& sx, int Dx,
                                              int x0, int xa, int ia, int ib, int& t0, int& t1, int& t2)
{
    auto fetch = [&](int i, int& c0, int& c1, int& c2) {
        const int rel = i - xa;
        if constexpr (FAM == CHIP_PACKED) {
            const uint8_t* q = L0 + (unsigned)rel * bpp;
            c0 = q[0]; c1 = q[1]; c2 = q[2];
        } else if constexpr (FAM == CHIP_PACKED32) {
            const unsigned int v = *reinterpret_cast<const unsigned int*>(L0 + (unsigned)rel * 4u);
            c0 = (int)(v & 0xffu); c1 = (int)((v >> 8) & 0xffu); c2 = (int)((v >> 16) & 0xffu);
        } else {
            unsigned int word;                                      // B | G << 8 | R << 16
            if constexpr (FAM == CHIP_YUV420) {
                const unsigned int Y = L0[rel];
                unsigned int uv;
                if (nv12) { const uint8_t* q = L1 + (rel & ~1); uv = (unsigned int)q[0] | ((unsigned int)q[1] << 8); }
                else uv = (unsigned int)L1[rel >> 1] | ((unsigned int)L2[rel >> 1] << 8);
                word = yuv_bgr_word(Y, uv, fmt);
            } else {
                const uint8_t* q = L0 + (rel & ~1) * 2;
                const int yo = (rel & 1) * 2;
                const bool uyvy = pix_is_uyvy(fmt);
                const unsigned int Y = uyvy ? q[1 + yo] : q[yo];
                const unsigned int uv = uyvy ? ((unsigned int)q[0] | ((unsigned int)q[2] << 8)) : ((unsigned int)q[1] | ((unsigned int)q[3] << 8));
                word = yuv_bgr_word(Y, uv, y422_matrix(fmt));
            }
            c0 = (int)(word & 0xffu); c1 = (int)((word >> 8) & 0xffu); c2 = (int)(word >> 16);
        }
    };
    int c0, c1, c2;
    if (ia <= ib && ia == x0 + sx.i0) {
        const int w = area_weight(sx, Dx, ia - x0);
        fetch(ia, c0, c1, c2);
        t0 += w * c0; t1 += w * c1; t2 += w * c2;
        ++ia;
    }
    if (ia <= ib && ib == x0 + sx.i1) {
        const int w = area_weight(sx, Dx, ib - x0);
        fetch(ib, c0, c1, c2);
        t0 += w * c0; t1 += w * c1; t2 += w * c2;
        --ib;
    }
    int s0 = 0, s1 = 0, s2 = 0;
#pragma unroll 2
    for (int i = ia; i <= ib; ++i) {
        fetch(i, c0, c1, c2);
        s0 += c0; s1 += c1; s2 += c2;
    }
    t0 += Dx * s0; t1 += Dx * s1; t2 += Dx * s2;
}

struct ChipCutArgs {
    const uint8_t* src; const ChipFrame* frames;
    uint8_t* chips;
    unsigned long long slab_bytes, pixels_off, chip_stride;
    int chip_w, chip_h, f32;
};

__global__ __launch_bounds__(ZLY_CHIP_THREADS) void chip_cut_kernel(ChipCutArgs A)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[2][3][CHIP_PLANE_LDS];
    const int tid = (int)threadIdx.x, band = (int)blockIdx.x, slot = (int)blockIdx.y, f = (int)blockIdx.z;
    uint8_t* const slab = A.chips + (size_t)f * A.slab_bytes;
    const zly_chip_header hd = *reinterpret_cast<const zly_chip_header*>(slab);
    if (slot >= hd.n_chips) return;                                 // uniform
    const zly_chip_rec rec = *reinterpret_cast<const zly_chip_rec*>(slab + chip_rec_off(slot));
    const ChipFrame F = A.frames[f];
    const int fmt = F.fmt, np = F.planes;
    const int x0 = rec.x0, y0 = rec.y0, Sx = rec.w, Sy = rec.h;
    const int Dx = A.chip_w, Dy = A.chip_h;
    // the select kernel writes legal rectangles only (chip_rect_axis); a record that is none is not followed: every address below is derived from it
    if (x0 < 0 || y0 < 0 || Sx < 1 || Sy < 1 || Sx > F.W - x0 || Sy > F.H - y0) return;

    const int y_first = band * ZLY_CHIP_BAND_ROWS, y_last = min(y_first + ZLY_CHIP_BAND_ROWS, Dy) - 1;
    const bool col_in = tid < Dx;                                   // this thread owns a chip column
    uint8_t* const chip = slab + A.pixels_off + (size_t)slot * A.chip_stride;

    // the frame columns and the rectangle's rows this workgroup reads
    const int xs0 = x0 & ~1, xs1 = x0 + Sx;
    const int js0 = area_span(Sy, Dy, y_first).i0, js1 = area_span(Sy, Dy, y_last).i1;
    const int nu = (xs1 - xs0 + ZLY_CHIP_CHUNK_PX - 1) / ZLY_CHIP_CHUNK_PX;        // staging units per row
    const int total = (js1 - js0 + 1) * nu;

    const AreaSpan sx = area_span(Sx, Dx, col_in ? tid : 0);
    const unsigned int T = (unsigned)Sx * (unsigned)Sy;
    const float inv_t = 1.0f / (float)T;

    const uint8_t* plo[3];
    const uint8_t* phi[3];
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) { plo[pl] = A.src + F.off[pl]; phi[pl] = plo[pl] + F.ext[pl]; }

    // the loads of unit u into registers: one 16-byte lane load per plane
    chip_u32x4 r[3] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
    auto issue = [&](int u) {
        const int j = js0 + u / nu, xa = xs0 + (u % nu) * ZLY_CHIP_CHUNK_PX, xb = min(xa + ZLY_CHIP_CHUNK_PX, xs1);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            if (pl >= np) continue;
            uint32_t nb;
            const uint8_t* g = A.src + chip_row_bytes(F, pl, y0 + j, xa, xb, &nb);
            const unsigned int sh = (unsigned int)((size_t)g & 15u);
            if ((unsigned)tid * 16u < sh + nb) r[pl] = chip_load16(g - sh + (size_t)tid * 16u, plo[pl], phi[pl]);
        }
    };

    int hs0 = 0, hs1 = 0, hs2 = 0;                                  // the current source row's horizontal sums: B, G, R
    unsigned long long a0 = 0, a1 = 0, a2 = 0;                      // the chip row in progress
    int y = y_first;
    AreaSpan sy = area_span(Sy, Dy, y);

    issue(0);
    for (int u = 0; u < total; ++u) {
        const int buf = u & 1;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
            if (pl < np) *reinterpret_cast<chip_u32x4*>(&lds[buf][pl][tid * 16]) = r[pl];
        __syncthreads();
        if (u + 1 < total) issue(u + 1);

        const int k = u % nu, j = js0 + u / nu, xa = xs0 + k * ZLY_CHIP_CHUNK_PX, xb = min(xa + ZLY_CHIP_CHUNK_PX, xs1);
        if (k == 0) { hs0 = 0; hs1 = 0; hs2 = 0; }
        if (col_in) {
            uint32_t nb;
            unsigned int sh[3] = {0u, 0u, 0u};
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                if (pl < np) sh[pl] = (unsigned int)((size_t)(A.src + chip_row_bytes(F, pl, y0 + j, xa, xb, &nb)) & 15u);
            const uint8_t* L0 = &lds[buf][0][sh[0]];
            const uint8_t* L1 = &lds[buf][1][sh[1]];
            const uint8_t* L2 = &lds[buf][2][sh[2]];
            const int ia = max(x0 + sx.i0, xa), ib = min(x0 + sx.i1, xb - 1);
            int p0 = 0, p1 = 0, p2 = 0;
            if (F.fam == ZLY_CHIP_FAM_NV12 || F.fam == ZLY_CHIP_FAM_I420)
                chip_row_sums<CHIP_YUV420>(L0, L1, L2, fmt, 1u, F.fam == ZLY_CHIP_FAM_NV12, sx, Dx, x0, xa, ia, ib, p0, p1, p2);
            else if (F.fam == ZLY_CHIP_FAM_Y422) chip_row_sums<CHIP_YUV422>(L0, L1, L2, fmt, 2u, false, sx, Dx, x0, xa, ia, ib, p0, p1, p2);
            else if (F.bpp == 4 && (sh[0] & 3u) == 0u) chip_row_sums<CHIP_PACKED32>(L0, L1, L2, fmt, 4u, false, sx, Dx, x0, xa, ia, ib, p0, p1, p2);
            else chip_row_sums<CHIP_PACKED>(L0, L1, L2, fmt, (unsigned)F.bpp, false, sx, Dx, x0, xa, ia, ib, p0, p1, p2);
            const bool swap = pix_is_rgb_order(fmt);                // the R-first layouts: the sums of byte 0 are R's
            hs0 += swap ? p2 : p0; hs1 += p1; hs2 += swap ? p0 : p2;
        }
        if (k != nu - 1) continue;
        // rectangle row j is complete: it belongs to the chip row in progress, and may end it and begin the next ones
        while (true) {
            const unsigned int wy = (unsigned int)area_weight(sy, Dy, j);
            a0 += (unsigned long long)wy * (unsigned int)hs0;
            a1 += (unsigned long long)wy * (unsigned int)hs1;
            a2 += (unsigned long long)wy * (unsigned int)hs2;
            if (j != sy.i1) break;
            if (col_in) {
                const unsigned int vb = chip_round_div(a0, T, inv_t), vg = chip_round_div(a1, T, inv_t), vr = chip_round_div(a2, T, inv_t);
                if (A.f32) {
                    float* o = reinterpret_cast<float*>(chip) + (size_t)y * Dx + tid;
                    const size_t plane = (size_t)Dx * Dy;
                    o[0] = (float)vr / 255.0f; o[plane] = (float)vg / 255.0f; o[2 * plane] = (float)vb / 255.0f;
                } else {
                    uint8_t* o = chip + ((size_t)y * Dx + tid) * 3;
                    o[0] = (uint8_t)vb; o[1] = (uint8_t)vg; o[2] = (uint8_t)vr;
                }
            }
            a0 = a1 = a2 = 0;
            if (++y > y_last) break;
            sy = area_span(Sy, Dy, y);
            if (sy.i0 != j) break;                                  // the next chip row begins with the next rectangle row
        }
    }
}

hipError_t launch_chips(const uint8_t* src, const ChipFrame* frames, int n, const void* slabs, size_t slab_bytes, int cap, void* chips, const zly_chip_config& cfg,
                        hipStream_t s)
{
    if (!src || !frames || !slabs || !chips || n < 1 || cfg.chip_w < 1 || cfg.chip_w > ZLY_CHIP_MAX_DIM || cfg.chip_h < 1 || cfg.chip_h > ZLY_CHIP_MAX_DIM ||
        cfg.max_chips < 1 || cfg.max_chips > cap)
        return hipErrorInvalidValue;
    const ChipLayout l = chip_layout(cfg.chip_w, cfg.chip_h, cfg.max_chips, cfg.layout == ZLY_CHIP_RGB_F32);
    hipLaunchKernelGGL(chip_select_kernel, dim3((unsigned)n), dim3(64), 0, s, (const uint8_t*)slabs, (unsigned long long)slab_bytes, cap, frames, (uint8_t*)chips,
                       (unsigned long long)l.slab_bytes, cfg.max_chips, cfg.class_id, cfg.scale);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    ChipCutArgs a;
    a.src = src; a.frames = frames; a.chips = (uint8_t*)chips;
    a.slab_bytes = l.slab_bytes; a.pixels_off = l.pixels_off; a.chip_stride = l.chip_stride;
    a.chip_w = cfg.chip_w; a.chip_h = cfg.chip_h; a.f32 = cfg.layout == ZLY_CHIP_RGB_F32 ? 1 : 0;
    const dim3 grid((unsigned)((cfg.chip_h + ZLY_CHIP_BAND_ROWS - 1) / ZLY_CHIP_BAND_ROWS), (unsigned)cfg.max_chips, (unsigned)n);
    hipLaunchKernelGGL(chip_cut_kernel, grid, dim3(ZLY_CHIP_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace zly

// nms_probe.hip -- TEST INFRASTRUCTURE (never part of libzly.so): one launch of the SHIPPED nms_kernel on candidate buffers the caller made.
// Linked against the very kernels_post.o that goes into libzly.so (Makefile: $(OUT)/libnms_probe.so, -Wl,-Bsymbolic so that its calls bind to
// its own copy when libzly.so lives in the same process); tests/test_gpu_nms_batched.py loads it with ctypes.  The launch has the production
// shape: n workgroups, frame f at cand + f*N, scratch + f*N and slabs + f*slab_bytes, counts reset by the kernel itself.
#include "zly_internal.h"
#include <stdint.h>
#include <string.h>

using namespace zly;

#define PROBE_TRY(x) do { hipError_t r_ = (x); if (r_ != hipSuccess && rc == hipSuccess) rc = r_; } while (0)

// cand: n*N Cand records, uploaded in full (stale tails behind each frame's count included); counts: n ints.
// scratch (n*N records) and slabs (n slabs + one guard slab) are filled with the given bytes before the launch.
// slabs_out: (n + 1) * (16 + 40*cap) bytes; counts_out: n ints and cand_out: n*N records as they are AFTER the launch.
// Returns the first HIP error code (0 = hipSuccess), or -1 for arguments the kernel must not be launched on.
extern "C" int nms_probe_run(const void* cand, const int* counts, int N, int n, float iou_thr, int nc, int cap, uint32_t tag0, int force_general,
                             int scratch_fill, int slab_fill, void* slabs_out, int* counts_out, void* cand_out)
{
    if (!cand || !counts || !slabs_out || !counts_out || !cand_out) return -1;
    if (N < 1 || n < 1 || n > 65535 || nc < 1 || nc > 1024 || cap < 1) return -1;
    const Cand* hc = static_cast<const Cand*>(cand);
    for (int f = 0; f < n; ++f) {                       // the kernel indexes LDS by the class of a live candidate: check on the host before it runs
        if (counts[f] < 0 || counts[f] > N) return -1;
        for (int i = 0; i < counts[f]; ++i) {
            const int c = hc[(size_t)f * N + i].cls;
            if (c < 0 || c >= nc) return -1;
        }
    }
    static bool inited = false;
    hipError_t rc = hipSuccess;
    if (!inited) { PROBE_TRY(nms_init()); if (rc != hipSuccess) return (int)rc; inited = true; }

    const size_t cand_bytes = (size_t)n * N * sizeof(Cand);
    const size_t slab_bytes = sizeof(zly_slab_header) + (size_t)cap * sizeof(zly_det);
    Cand *d_cand = nullptr, *d_scratch = nullptr;
    int* d_count = nullptr;
    unsigned char* d_slabs = nullptr;
    hipStream_t s = nullptr;
    PROBE_TRY(hipMalloc((void**)&d_cand, cand_bytes));
    PROBE_TRY(hipMalloc((void**)&d_scratch, cand_bytes));
    PROBE_TRY(hipMalloc((void**)&d_count, (size_t)n * sizeof(int)));
    PROBE_TRY(hipMalloc((void**)&d_slabs, (size_t)(n + 1) * slab_bytes));
    PROBE_TRY(hipStreamCreate(&s));
    if (rc == hipSuccess) {
        PROBE_TRY(hipMemcpyAsync(d_cand, cand, cand_bytes, hipMemcpyHostToDevice, s));
        PROBE_TRY(hipMemcpyAsync(d_count, counts, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
        PROBE_TRY(hipMemsetAsync(d_scratch, scratch_fill & 0xff, cand_bytes, s));
        PROBE_TRY(hipMemsetAsync(d_slabs, slab_fill & 0xff, (size_t)(n + 1) * slab_bytes, s));
    }
    if (rc == hipSuccess) PROBE_TRY(launch_nms(d_cand, d_count, N, n, iou_thr, nc, d_scratch, d_slabs, cap, tag0, s, force_general));
    if (rc == hipSuccess) PROBE_TRY(hipStreamSynchronize(s));
    if (rc == hipSuccess) {
        PROBE_TRY(hipMemcpy(slabs_out, d_slabs, (size_t)(n + 1) * slab_bytes, hipMemcpyDeviceToHost));
        PROBE_TRY(hipMemcpy(counts_out, d_count, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
        PROBE_TRY(hipMemcpy(cand_out, d_cand, cand_bytes, hipMemcpyDeviceToHost));
    }
    if (s) PROBE_TRY(hipStreamDestroy(s));
    if (d_cand) PROBE_TRY(hipFree(d_cand));
    if (d_scratch) PROBE_TRY(hipFree(d_scratch));
    if (d_count) PROBE_TRY(hipFree(d_count));
    if (d_slabs) PROBE_TRY(hipFree(d_slabs));
    return (int)rc;
}

extern "C" int nms_probe_sizeof_cand(void) { return (int)sizeof(Cand); }

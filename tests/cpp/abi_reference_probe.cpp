// abi_reference_probe.cpp -- prints, as one JSON object, the layout of the REFERENCE's zero_latency::Detection (src/common/types.h)
// or, built with -DPROBE_RESULT, the values of its zero_latency::ErrorCode (src/common/result.h).  The two headers declare
// conflicting ErrorCode enums (types.h:84, one of the reasons the reference does not compile as a whole: SURVEY F3), hence two builds.
// Run by tests/golden/make_abi_golden.py against a reference tree (-I <reference>/src/common); its output is committed as
// tests/golden/reference_abi.json, which tests/test_abi.py checks include/zly.h against with the compiler.  Nothing of the
// reference is copied here: this file only names its types.
#include <cstddef>
#include <cstdio>
#ifdef PROBE_RESULT
#include "result.h"         // the reference's, via -I <reference>/src/common
using zero_latency::ErrorCode;
#define CODE(n) std::printf("%s\"%s\": %d", first ? "" : ", ", #n, (int)ErrorCode::n), first = false
int main() {
    bool first = true;
    std::printf("{\"ErrorCode\": {");
    CODE(OK); CODE(INVALID_ARGUMENT); CODE(NOT_INITIALIZED); CODE(INFERENCE_ERROR); CODE(MODEL_NOT_FOUND); CODE(MODEL_LOAD_FAILED);
    CODE(INVALID_INPUT); CODE(SYSTEM_ERROR);
    std::printf("}}\n");
    return 0;
}
#else
#include "types.h"          // the reference's, via -I <reference>/src/common
using RefDet = zero_latency::Detection;
using RefBox = zero_latency::BoundingBox;
using RefState = zero_latency::GameState;
int main() {
    std::printf("{\"Detection\": {\"sizeof\": %zu, \"alignof\": %zu, \"offsetof\": {\"box\": %zu, \"box.x\": %zu, \"box.y\": %zu, \"box.width\": %zu, "
                "\"box.height\": %zu, \"confidence\": %zu, \"class_id\": %zu, \"track_id\": %zu, \"timestamp\": %zu}, "
                "\"sizeof_member\": {\"class_id\": %zu, \"timestamp\": %zu}}, ",
                sizeof(RefDet), alignof(RefDet), offsetof(RefDet, box), offsetof(RefDet, box) + offsetof(RefBox, x),
                offsetof(RefDet, box) + offsetof(RefBox, y), offsetof(RefDet, box) + offsetof(RefBox, width),
                offsetof(RefDet, box) + offsetof(RefBox, height), offsetof(RefDet, confidence), offsetof(RefDet, class_id),
                offsetof(RefDet, track_id), offsetof(RefDet, timestamp), sizeof(RefDet::class_id), sizeof(RefDet::timestamp));
    // GameState: the members the plugin fills (frame_id, timestamp, detections)
    std::printf("\"GameState\": {\"sizeof_member\": {\"frame_id\": %zu, \"timestamp\": %zu, \"detections_element\": %zu}}}\n",
                sizeof(RefState::frame_id), sizeof(RefState::timestamp), sizeof(decltype(RefState::detections)::value_type));
    return 0;
}
#endif

# Build recipe for the MI355X-native detect engine (gfx950 only) and its test infrastructure.
#   make            -> libzly.so (HIP engine + C ABI), libzly_plugin.so (IInferenceEngine host side),
#                      host test binary, CPU oracle, synthetic weight files
#   make oracle     -> oracle/_build/libzly_oracle.so only (gcc, no GPU toolchain needed)
PKG      := zero-latency-yolo_amd
CSRC     := $(PKG)/csrc
HOST     := $(PKG)/host
OUT      := $(PKG)/_build
HIPCC    ?= hipcc
ARCH     ?= gfx950
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Iinclude -I$(CSRC) -Wall -Wno-unused-function -Wno-unused-result -Wno-unused-value
CXX      ?= g++
PY       ?= python3

KERNELS  := $(CSRC)/kernels_conv.hip $(CSRC)/kernels_pair.hip $(CSRC)/kernels_misc.hip $(CSRC)/kernels_head.hip $(CSRC)/kernels_stem.hip $(CSRC)/kernels_stem_yuv.hip $(CSRC)/kernels_lb.hip $(CSRC)/kernels_view.hip $(CSRC)/kernels_pix.hip $(CSRC)/kernels_pix_view.hip $(CSRC)/kernels_y422.hip $(CSRC)/kernels_y422_view.hip $(CSRC)/kernels_post.hip $(CSRC)/kernels_c2f64.hip $(CSRC)/kernels_sppf.hip $(CSRC)/kernels_track.hip $(CSRC)/kernels_merge.hip $(CSRC)/kernels_area.hip $(CSRC)/kernels_surface.hip $(CSRC)/kernels_zoom.hip $(CSRC)/kernels_chips.hip $(CSRC)/kernels_change.hip $(CSRC)/kernels_camera.hip
ENGINE   := $(CSRC)/engine.cpp $(CSRC)/weights.cpp
OBJS     := $(OUT)/kernels_conv.o $(OUT)/kernels_pair.o $(OUT)/kernels_misc.o $(OUT)/kernels_head.o $(OUT)/kernels_stem.o $(OUT)/kernels_stem_yuv.o $(OUT)/kernels_lb.o $(OUT)/kernels_view.o $(OUT)/kernels_pix.o $(OUT)/kernels_pix_view.o $(OUT)/kernels_y422.o $(OUT)/kernels_y422_view.o $(OUT)/kernels_post.o $(OUT)/kernels_c2f64.o $(OUT)/kernels_sppf.o $(OUT)/kernels_track.o $(OUT)/kernels_merge.o $(OUT)/kernels_area.o $(OUT)/kernels_surface.o $(OUT)/kernels_zoom.o $(OUT)/kernels_chips.o $(OUT)/kernels_change.o $(OUT)/kernels_camera.o $(OUT)/engine.o $(OUT)/weights.o

all: $(OUT)/libzly.so $(OUT)/libzly_gather.so $(OUT)/test_gather $(OUT)/zly_sharded_bench $(OUT)/libnms_probe.so $(OUT)/libsppf_probe.so $(OUT)/libtrack_probe.so oracle weights host

$(OUT):
	mkdir -p $(OUT)

KHDRS    := $(CSRC)/zly_internal.h $(CSRC)/front_variants.h $(CSRC)/conv_device.h $(CSRC)/yuv_device.h $(CSRC)/letterbox_device.h $(CSRC)/planes_device.h $(CSRC)/area_device.h $(CSRC)/surface_device.h $(CSRC)/chip_device.h $(CSRC)/change_device.h $(CSRC)/camera_device.h $(CSRC)/head_skip.h include/zly.h
$(OUT)/%.o: $(CSRC)/%.hip $(KHDRS) | $(OUT)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

# the side units of the front kernels (front_variants.h) compile the main units' text
$(OUT)/kernels_stem_yuv.o: $(CSRC)/kernels_stem.hip
$(OUT)/kernels_lb.o: $(CSRC)/kernels_misc.hip $(CSRC)/kernels_stem.hip $(CSRC)/kernels_head.hip
$(OUT)/kernels_view.o $(OUT)/kernels_pix.o $(OUT)/kernels_pix_view.o $(OUT)/kernels_y422.o $(OUT)/kernels_y422_view.o: $(CSRC)/kernels_misc.hip $(CSRC)/kernels_stem.hip
# the plan kernel of the zoom regions compiles the arithmetic it shares with the host twin
$(OUT)/kernels_zoom.o: $(CSRC)/zoom_device.h
# ... and the change map's kernels the arithmetic of the zoom regions' size and plane offsets
$(OUT)/kernels_change.o: $(CSRC)/zoom_device.h
# ... and the camera motion's kernels the change map's arithmetic, which includes it
$(OUT)/kernels_camera.o: $(CSRC)/zoom_device.h

ENGINE_DEPS := $(CSRC)/engine.cpp $(CSRC)/zly_internal.h $(CSRC)/front_variants.h $(CSRC)/frame_rules.h $(CSRC)/surface_rules.h $(CSRC)/surface_device.h $(CSRC)/zoom_rules.h $(CSRC)/zoom_device.h $(CSRC)/chip_rules.h $(CSRC)/chip_device.h $(CSRC)/change_rules.h $(CSRC)/change_device.h $(CSRC)/camera_rules.h $(CSRC)/camera_device.h $(CSRC)/upload_ring.h $(CSRC)/weights.h include/zly.h
$(OUT)/engine.o: $(ENGINE_DEPS) | $(OUT)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

$(OUT)/weights.o: $(CSRC)/weights.cpp $(CSRC)/weights.h include/zly.h | $(OUT)
	$(HIPCC) $(HIPFLAGS) -x hip -c $< -o $@

$(OUT)/libzly.so: $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS)

# ---- diagnostic build of the engine (never shipped, never loaded by tests / bench.py / the plugin): the same kernels, engine.cpp with -DZLY_DIAG, which
#      compiles in the result-changing ZLY_ABLATE_SKIP switch of tools/ablate_launches.sh (ZLY_LIB=.../libzly_diag.so python3 bench.py ...)
diaglib: $(OUT)/libzly_diag.so
$(OUT)/engine_diag.o: $(ENGINE_DEPS) | $(OUT)
	$(HIPCC) $(HIPFLAGS) -DZLY_DIAG=1 -x hip -c $< -o $@
$(OUT)/libzly_diag.so: $(filter-out $(OUT)/engine.o,$(OBJS)) $(OUT)/engine_diag.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

# ---- test infrastructure: one batched launch of the shipped nms_kernel on caller-made candidate buffers (tests/test_gpu_nms_batched.py).  It links the
#      kernels_post.o of libzly.so itself -- the object under test, not a recompilation; -Bsymbolic: its calls bind to its own copy beside libzly.so
nms_probe: $(OUT)/libnms_probe.so
$(OUT)/nms_probe_main.o: tests/cpp/nms_probe.hip $(CSRC)/zly_internal.h include/zly.h | $(OUT)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(OUT)/libnms_probe.so: $(OUT)/nms_probe_main.o $(OUT)/kernels_post.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -Wl,-Bsymbolic -o $@ $^

# ---- test infrastructure: single launches of the shipped SPPF kernels (the two pool kernels, the fused block) on caller-made buffers
#      (tests/test_gpu_sppf.py).  As above: the kernels_misc.o, kernels_sppf.o and weights.o of libzly.so itself, not recompilations
sppf_probe: $(OUT)/libsppf_probe.so
$(OUT)/sppf_probe_main.o: tests/cpp/sppf_probe.hip $(CSRC)/zly_internal.h $(CSRC)/weights.h include/zly.h | $(OUT)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(OUT)/sppf_probe_y422.o: tests/cpp/sppf_probe_y422.hip $(CSRC)/zly_internal.h $(CSRC)/front_variants.h include/zly.h | $(OUT)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(OUT)/libsppf_probe.so: $(OUT)/sppf_probe_main.o $(OUT)/sppf_probe_y422.o $(OUT)/kernels_misc.o $(OUT)/kernels_sppf.o $(OUT)/weights.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -Wl,-Bsymbolic -o $@ $^

# ---- test infrastructure: single launches of the shipped zoom plan kernel and the two tracking kernels on caller-made track tables, descriptor blocks,
#      merge tables and slabs (tests/test_gpu_track_tables.py).  As above: the kernels_track.o and kernels_zoom.o of libzly.so itself, not recompilations
track_probe: $(OUT)/libtrack_probe.so
$(OUT)/track_probe_main.o: tests/cpp/track_probe.hip $(CSRC)/zly_internal.h $(CSRC)/front_variants.h $(CSRC)/zoom_rules.h $(CSRC)/zoom_device.h $(CSRC)/frame_rules.h include/zly.h | $(OUT)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
$(OUT)/libtrack_probe.so: $(OUT)/track_probe_main.o $(OUT)/kernels_track.o $(OUT)/kernels_zoom.o
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -Wl,-Bsymbolic -o $@ $^

# ---- in-process RCCL gather of result slabs (include/zly_gather.h): a library of its own -- it links RCCL, and a process that already carries
#      PyTorch's bundled RCCL (bench.py, the tests) must never load a second one
$(OUT)/libzly_gather.so: $(CSRC)/gather.cpp include/zly_gather.h | $(OUT)
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 -fPIC -shared -Iinclude -x hip $(CSRC)/gather.cpp -o $@ -L/opt/rocm/lib -lrccl

$(OUT)/test_gather: tests/cpp/test_gather.cpp $(OUT)/libzly_gather.so $(OUT)/libzly.so
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 -Wno-unused-value -Iinclude -x hip tests/cpp/test_gather.cpp -o $@ -L$(OUT) -lzly_gather -lzly -Wl,-rpath,'$$ORIGIN'

# the product caller of the gather library: one process, N GPUs in lock step (host/zly_sharded.hpp), as a bench / check tool
$(OUT)/zly_sharded_bench: $(PKG)/tools/bench_sharded.cpp $(HOST)/zly_sharded.hpp $(HOST)/zly_sharded_hip.hpp $(HOST)/zly_compat.hpp include/zly.h include/zly_gather.h $(OUT)/libzly_gather.so $(OUT)/libzly.so
	$(HIPCC) --offload-arch=$(ARCH) -O2 -std=c++17 -Wno-unused-value -Iinclude -I$(HOST) -x hip $(PKG)/tools/bench_sharded.cpp -o $@ -L$(OUT) -lzly_gather -lzly -Wl,-rpath,'$$ORIGIN'

# ... and its host logic against stubs of both C ABIs and of the device runtime (test infrastructure: no GPU, no libzly.so)
$(OUT)/test_sharded_stub: tests/cpp/test_sharded_stub.cpp $(HOST)/zly_sharded.hpp $(HOST)/zly_compat.hpp include/zly.h include/zly_gather.h | $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -I$(HOST) -o $@ tests/cpp/test_sharded_stub.cpp

# ---- host side: the reference's IInferenceEngine plugin interface over the C ABI -----------------
host: $(OUT)/libzly_plugin.so $(OUT)/test_hip_engine $(OUT)/test_hip_engine_yuv $(OUT)/test_hip_engine_pix $(OUT)/test_wire $(OUT)/test_game_step $(OUT)/test_head_skip $(OUT)/test_frame_server $(OUT)/zly_h2h_bench $(OUT)/test_plugin_stub $(OUT)/test_plugin_crop_stub $(OUT)/test_plugin_yuv422_stub $(OUT)/test_plugin_track_stub $(OUT)/test_plugin_track_stub_nosym $(OUT)/test_plugin_track_motion_stub $(OUT)/test_plugin_track_motion_stub_nosym $(OUT)/test_plugin_area_stub $(OUT)/test_area_footprint $(OUT)/test_frame_rules $(OUT)/test_surface_rules $(OUT)/test_surface_moves $(OUT)/test_zoom_plan $(OUT)/test_chip_rules $(OUT)/test_change_rules $(OUT)/test_camera_rules $(OUT)/test_sharded_stub

$(OUT)/libzly_plugin.so: $(HOST)/hip_inference_engine.cpp $(HOST)/hip_inference_engine.h $(HOST)/zly_sha256.hpp $(HOST)/zly_compat.hpp include/zly.h $(OUT)/libzly.so
	$(CXX) -O2 -std=c++17 -fPIC -shared -Iinclude -I$(HOST) -o $@ $(HOST)/hip_inference_engine.cpp -L$(OUT) -lzly -pthread -Wl,-rpath,'$$ORIGIN'

$(OUT)/test_hip_engine: tests/cpp/test_hip_engine.cpp $(OUT)/libzly_plugin.so
	$(CXX) -O2 -std=c++17 -Iinclude -I$(HOST) -o $@ tests/cpp/test_hip_engine.cpp -Wl,--no-as-needed -L$(OUT) -lzly_plugin -lzly -pthread -Wl,-rpath,'$$ORIGIN'

$(OUT)/test_hip_engine_yuv: tests/cpp/test_hip_engine_yuv.cpp $(OUT)/libzly_plugin.so
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -I$(HOST) -o $@ tests/cpp/test_hip_engine_yuv.cpp -Wl,--no-as-needed -L$(OUT) -lzly_plugin -lzly -pthread -Wl,-rpath,'$$ORIGIN'

$(OUT)/test_hip_engine_pix: tests/cpp/test_hip_engine_pix.cpp $(OUT)/libzly_plugin.so
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -I$(HOST) -o $@ tests/cpp/test_hip_engine_pix.cpp -Wl,--no-as-needed -L$(OUT) -lzly_plugin -lzly -pthread -Wl,-rpath,'$$ORIGIN'

$(OUT)/zly_h2h_bench: $(PKG)/tools/bench_h2h.cpp $(OUT)/libzly_plugin.so
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -I$(HOST) -o $@ $(PKG)/tools/bench_h2h.cpp -Wl,--no-as-needed -L$(OUT) -lzly_plugin -lzly -pthread -Wl,-rpath,'$$ORIGIN'

$(OUT)/test_frame_server: tests/cpp/test_frame_server.cpp $(HOST)/zly_frame_server.hpp $(HOST)/zly_wire.hpp $(HOST)/zly_game_step.hpp $(OUT)/libzly_plugin.so
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -I$(HOST) -o $@ tests/cpp/test_frame_server.cpp -Wl,--no-as-needed -L$(OUT) -lzly_plugin -lzly -pthread -Wl,-rpath,'$$ORIGIN'

# the plugin's host logic against a link-time stub of the C ABI (test infrastructure: no libzly.so, no GPU)
$(OUT)/test_plugin_stub: tests/cpp/test_plugin_stub.cpp $(HOST)/hip_inference_engine.cpp $(HOST)/hip_inference_engine.h $(HOST)/zly_compat.hpp include/zly.h | $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -I$(HOST) -o $@ tests/cpp/test_plugin_stub.cpp -pthread

# ... and five more sides of it against one shared stub (tests/cpp/plugin_abi_stub.hpp), whose frame and view checks are the product's own (csrc/frame_rules.h):
ABI_STUB := tests/cpp/plugin_abi_stub.hpp $(CSRC)/frame_rules.h $(CSRC)/front_variants.h $(HOST)/hip_inference_engine.cpp $(HOST)/hip_inference_engine.h $(HOST)/zly_compat.hpp include/zly.h
# its ZLY_CROP logic, from the frame views the stub records
$(OUT)/test_plugin_crop_stub: tests/cpp/test_plugin_crop_stub.cpp $(ABI_STUB) | $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -I$(HOST) -I$(CSRC) -o $@ tests/cpp/test_plugin_crop_stub.cpp -pthread

# ... and its packed YUV 4:2:2 input formats (names, sizes, ZLY_CROP's x-only evenness rule) against a stub of the same kind
$(OUT)/test_plugin_yuv422_stub: tests/cpp/test_plugin_yuv422_stub.cpp $(ABI_STUB) | $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -I$(HOST) -I$(CSRC) -o $@ tests/cpp/test_plugin_yuv422_stub.cpp -pthread

# ... and its ZLY_TRACK logic against a stub that records (engine, stream) of every submit and every reset; the second binary's stub lacks the tracking calls
$(OUT)/test_plugin_track_stub: tests/cpp/test_plugin_track_stub.cpp $(ABI_STUB) | $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -I$(HOST) -I$(CSRC) -o $@ tests/cpp/test_plugin_track_stub.cpp -pthread
$(OUT)/test_plugin_track_stub_nosym: tests/cpp/test_plugin_track_stub.cpp $(ABI_STUB) | $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -DNO_TRACK_SYMBOLS -Iinclude -I$(HOST) -I$(CSRC) -o $@ tests/cpp/test_plugin_track_stub.cpp -pthread

# ... and its ZLY_TRACK_MOTION logic against a stub that records the enables; the second binary's stub has the tracking calls but not the motion model's
$(OUT)/test_plugin_track_motion_stub: tests/cpp/test_plugin_track_motion_stub.cpp $(ABI_STUB) | $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -I$(HOST) -I$(CSRC) -o $@ tests/cpp/test_plugin_track_motion_stub.cpp -pthread
$(OUT)/test_plugin_track_motion_stub_nosym: tests/cpp/test_plugin_track_motion_stub.cpp $(ABI_STUB) | $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -DNO_MOTION_SYMBOLS -Iinclude -I$(HOST) -I$(CSRC) -o $@ tests/cpp/test_plugin_track_motion_stub.cpp -pthread

# ... and its ZLY_RESIZE names (stretch, letterbox, area, letterbox_area) against a stub that records the zly_config it is handed
$(OUT)/test_plugin_area_stub: tests/cpp/test_plugin_area_stub.cpp $(ABI_STUB) | $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -I$(HOST) -I$(CSRC) -o $@ tests/cpp/test_plugin_area_stub.cpp -pthread

# the area resize filter's per-axis footprint arithmetic (csrc/area_device.h) as the pre-pass kernel computes it, printed for tests/test_area_footprint.py (test infrastructure: no GPU)
$(OUT)/test_area_footprint: tests/cpp/test_area_footprint.cpp $(CSRC)/area_device.h | $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -I$(CSRC) -o $@ tests/cpp/test_area_footprint.cpp

# the frame and view rules (csrc/frame_rules.h) on their own, for tests/test_frame_rules.py (test infrastructure: no GPU, nothing of the engine) ...
$(OUT)/test_frame_rules: tests/cpp/test_frame_rules.cpp $(CSRC)/frame_rules.h $(CSRC)/front_variants.h include/zly.h | $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -I$(CSRC) -o $@ tests/cpp/test_frame_rules.cpp
# ... and under the host sanitizers: not part of `all`; make frame_rules_san && $(OUT)/test_frame_rules_san
frame_rules_san: $(OUT)/test_frame_rules_san
$(OUT)/test_frame_rules_san: tests/cpp/test_frame_rules.cpp $(CSRC)/frame_rules.h $(CSRC)/front_variants.h include/zly.h | $(OUT)
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -I$(CSRC) -o $@ tests/cpp/test_frame_rules.cpp

# the rules of the resident surfaces (csrc/surface_rules.h: refusals, job and band tables) on their own, for tests/test_surface_rules.py: the program also
# EXECUTES a table with memcpy on host arrays (test infrastructure: no GPU, nothing of the engine) ...
SURFACE_RULES := tests/cpp/test_surface_rules.cpp $(CSRC)/surface_rules.h $(CSRC)/surface_device.h $(CSRC)/frame_rules.h $(CSRC)/front_variants.h include/zly.h
$(OUT)/test_surface_rules: $(SURFACE_RULES) | $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -I$(CSRC) -o $@ tests/cpp/test_surface_rules.cpp
# ... and under the host sanitizers: not part of `all`; make surface_rules_san && $(OUT)/test_surface_rules_san selftest
surface_rules_san: $(OUT)/test_surface_rules_san
$(OUT)/test_surface_rules_san: $(SURFACE_RULES) | $(OUT)
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -I$(CSRC) -o $@ tests/cpp/test_surface_rules.cpp
# the moves of the resident surfaces (csrc/surface_rules.h: surface_plan_moves -- refusals, phases, tables) on their own, for tests/test_surface_moves.py:
# the program executes every launch's bands item by item as the kernels walk them, in three orders
SURFACE_MOVES := tests/cpp/test_surface_moves.cpp $(CSRC)/surface_rules.h $(CSRC)/surface_device.h $(CSRC)/frame_rules.h $(CSRC)/front_variants.h include/zly.h
$(OUT)/test_surface_moves: $(SURFACE_MOVES) | $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -Iinclude -I$(CSRC) -o $@ tests/cpp/test_surface_moves.cpp
# ... and under the host sanitizers: not part of `all`; make surface_moves_san, then run it on a script
surface_moves_san: $(OUT)/test_surface_moves_san
$(OUT)/test_surface_moves_san: $(SURFACE_MOVES) | $(OUT)
	$(CXX) -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -I$(CSRC) -o $@ tests/cpp/test_surface_moves.cpp

# the plan of the zoom regions (csrc/zoom_device.h through the host twin of csrc/zoom_rules.h) on its own, for tests/test_zoom_plan.py: the program reads track
# tables and prints plans, and walks the per-plane offset arithmetic against view_crop (test infrastructure: no GPU, nothing of the engine).  Contraction
# off, as in the kernel's unit ...
ZOOM_PLAN := tests/cpp/test_zoom_plan.cpp $(CSRC)/zoom_rules.h $(CSRC)/zoom_device.h $(CSRC)/frame_rules.h $(CSRC)/front_variants.h include/zly.h
$(OUT)/test_zoom_plan: $(ZOOM_PLAN) | $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -ffp-contract=off -Iinclude -I$(CSRC) -o $@ tests/cpp/test_zoom_plan.cpp
# ... and under the host sanitizers: not part of `all`; make zoom_plan_san && $(OUT)/test_zoom_plan_san selftest
zoom_plan_san: $(OUT)/test_zoom_plan_san
$(OUT)/test_zoom_plan_san: $(ZOOM_PLAN) | $(OUT)
	$(CXX) -O1 -g -std=c++17 -Wall -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -I$(CSRC) -o $@ tests/cpp/test_zoom_plan.cpp

# the chips' rules (csrc/chip_device.h, csrc/chip_rules.h) on their own, for tests/test_chip_rules.py: the program reads (view, slab, config) scripts,
# prints the records and cuts the chips pixel by pixel through the header's addressing, counting every sample address outside its plane's extent
# (test infrastructure: no GPU, nothing of the engine).  Contraction off, as in the kernels' unit ...
CHIP_RULES := tests/cpp/test_chip_rules.cpp $(CSRC)/chip_rules.h $(CSRC)/chip_device.h $(CSRC)/area_device.h $(CSRC)/frame_rules.h $(CSRC)/front_variants.h include/zly.h
chip_rules: $(OUT)/test_chip_rules
$(OUT)/test_chip_rules: $(CHIP_RULES) | $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -ffp-contract=off -Iinclude -I$(CSRC) -o $@ tests/cpp/test_chip_rules.cpp
# ... and under the host sanitizers: not part of `all`; make chip_rules_san, then run it on a script
chip_rules_san: $(OUT)/test_chip_rules_san
$(OUT)/test_chip_rules_san: $(CHIP_RULES) | $(OUT)
	$(CXX) -O1 -g -std=c++17 -Wall -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -I$(CSRC) -o $@ tests/cpp/test_chip_rules.cpp

# the change map's rules (csrc/change_device.h, csrc/change_rules.h) on their own, for tests/test_change_rules.py: the program reads (view, config) scripts,
# computes the sums through the kernel's own addressing, counting every needed sample address outside its plane's extent, and prints the records of
# the host twin of the pick kernel and of the zoom fill (test infrastructure: no GPU, nothing of the engine) ...
CHANGE_RULES := tests/cpp/test_change_rules.cpp $(CSRC)/change_rules.h $(CSRC)/change_device.h $(CSRC)/chip_rules.h $(CSRC)/chip_device.h $(CSRC)/zoom_rules.h $(CSRC)/zoom_device.h $(CSRC)/frame_rules.h $(CSRC)/front_variants.h include/zly.h
change_rules: $(OUT)/test_change_rules
$(OUT)/test_change_rules: $(CHANGE_RULES) | $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -ffp-contract=off -Iinclude -I$(CSRC) -o $@ tests/cpp/test_change_rules.cpp
# ... and under the host sanitizers: not part of `all`; make change_rules_san, then run it on a script
change_rules_san: $(OUT)/test_change_rules_san
$(OUT)/test_change_rules_san: $(CHANGE_RULES) | $(OUT)
	$(CXX) -O1 -g -std=c++17 -Wall -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -I$(CSRC) -o $@ tests/cpp/test_change_rules.cpp

# the camera motion's rules (csrc/camera_device.h, csrc/camera_rules.h) on their own, for tests/test_camera_rules.py: the program reads (view, config)
# scripts, computes the sums through the change map's host twin and prints the records of the host twin of the search, pick and apply kernels
# (test infrastructure: no GPU, nothing of the engine).  Contraction off, as in the kernels' unit ...
CAMERA_RULES := tests/cpp/test_camera_rules.cpp $(CSRC)/camera_rules.h $(CSRC)/camera_device.h $(filter-out tests/cpp/test_change_rules.cpp,$(CHANGE_RULES))
camera_rules: $(OUT)/test_camera_rules
$(OUT)/test_camera_rules: $(CAMERA_RULES) | $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -ffp-contract=off -Iinclude -I$(CSRC) -o $@ tests/cpp/test_camera_rules.cpp
# ... and under the host sanitizers: not part of `all`; make camera_rules_san, then run it on a script
camera_rules_san: $(OUT)/test_camera_rules_san
$(OUT)/test_camera_rules_san: $(CAMERA_RULES) | $(OUT)
	$(CXX) -O1 -g -std=c++17 -Wall -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -I$(CSRC) -o $@ tests/cpp/test_camera_rules.cpp

$(OUT)/test_wire: tests/cpp/test_wire.cpp $(HOST)/zly_wire.hpp $(HOST)/zly_sha256.hpp $(HOST)/zly_compat.hpp | $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -I$(HOST) -o $@ tests/cpp/test_wire.cpp

$(OUT)/test_game_step: tests/cpp/test_game_step.cpp $(HOST)/zly_game_step.hpp $(HOST)/zly_compat.hpp | $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -I$(HOST) -o $@ tests/cpp/test_game_step.cpp

# the Detect tail's early-out bound (csrc/head_skip.h) as the launcher computes it, printed for tests/test_head_skip.py (test infrastructure: no GPU)
$(OUT)/test_head_skip: tests/cpp/test_head_skip.cpp $(CSRC)/head_skip.h | $(OUT)
	$(CXX) -O2 -std=c++17 -Wall -I$(CSRC) -o $@ tests/cpp/test_head_skip.cpp

# ---- CPU oracle (test infrastructure only) --------------------------------------------------------
oracle: oracle/_build/libzly_oracle.so

oracle/_build/libzly_oracle.so: oracle/zly_oracle.c
	mkdir -p oracle/_build
	gcc -O2 -ffp-contract=off -fno-fast-math -shared -fPIC -o $@ $<

# ---- seeded synthetic weights (no real weights exist offline) --------------------------------------
weights: $(OUT)/yolov8n_synth.zlyw

$(OUT)/yolov8n_synth.zlyw: $(PKG)/tools/zly_model.py | $(OUT)
	$(PY) $(PKG)/tools/zly_model.py --scale n -o $@

# ---- diagnostic build of the LDS conv kernel with s_memtime stamps per phase (never linked into libzly.so) --------
diag: $(OUT)/diag_lds

$(OUT)/diag_lds: $(PKG)/tools/diag_lds.hip $(CSRC)/kernels_conv.hip $(CSRC)/zly_internal.h $(CSRC)/front_variants.h | $(OUT)
	$(HIPCC) $(HIPFLAGS) -DZLY_DIAG=1 $< -o $@

clean:
	rm -rf $(OUT) oracle/_build

.PHONY: all host oracle weights diag diaglib nms_probe sppf_probe track_probe frame_rules_san surface_rules_san surface_moves_san zoom_plan_san chip_rules chip_rules_san change_rules change_rules_san camera_rules camera_rules_san clean

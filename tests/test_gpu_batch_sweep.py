"""Every batch size a 64-frame engine resolves (run on the MI355X box: pytest -m gpu).  resolve_launches builds one launch table per batch size n, and
nearly everything in it depends on n: the C2f and bottleneck-pair tile shapes, the weight-stationary / LDS / stream / direct conv plans and their
split-K, the merged Detect launches (n <= 4), the side lanes with per-level tails and the deferred NMS (n >= 16), the tail's box conv.  The rest of the
suite runs n in {1, 2, 3, 4, 5, 8, 16, 32, 64}; the pipelined host path hands an engine any n up to max_batch.  Nothing here has a tolerance of its own:
the per-element bound and the decode tolerances are those of tests/closed_loop_ref.py (C_ACC, DECODE_*_TOL), everything else is equality of bytes.
References: float64 on the CPU on the engine's own tapped inputs, the oracle's post-processing of the engine's own head tensor, or the bytes of a
differently configured engine / call -- never the path under test itself.  What the shapes are for:
  * YOLOv8n at 416 x 416, n = 1 .. 64 (FLAG_DUMP_LOGITS, zly_detect_device so the front kernel runs): the headline's shape; every planned tile shape
    of the four fused C2f blocks, the two carried pixel tiles per wave of the 16-wave back half of model.4, every split-K and persistent-loop
    remainder, both sides of n <= 4 and n >= 16.  Frames 0 and n - 1 are checked (the last frame sits in the last, partial round of every tile loop);
  * YOLOv8n at 352 x 288, n = 1 .. 64: ragged 88 x 72 .. 11 x 9 maps, so every planned tile shape meets partial tiles on the right and bottom edges
    and M = n H W is no multiple of anything (the direct kernel's reciprocal pixel indexing, the stream kernel's group count);
  * YOLOv8-s at 352 x 288, n = 1 .. 32: other widths, conv3x3_ws_pair_kernel, the 64-channel C2f kernel;
  * the production flags (FLAG_NO_HEAD_TENSOR | FLAG_ASYNC_NMS, graphs on; what bench.py and the plugin run) at 416 x 416 must give the dump engine's
    slabs at every n: the closed-loop checks speak about production only through this equality.  On that engine every n is visited in three
    different shuffled orders (capture, then replay; other neighbours; deferred and joined NMS interleaved; the third time queued back to back
    without a host synchronisation) and must give the same bytes -- stale split-K accumulators, counters, candidate-buffer parity, descriptor
    caching -- and six odd sizes must be permutation equivariant bit for bit;
  * max_batch = 24 through zly_submit / zly_wait from four threads with nine frames of mixed sizes: the bf16 engine's partial batches launch eagerly
    from cached kernel shapes.  Every ticket must equal its frame's result inside a batch of SOME n, taken from a second engine's synchronous path.
test_coverage_is_recorded asserts from op_kernels what the sweep reached, and prints n -> launch table id, the tile shapes per fused block and the
pixel tiles a wave carries, so a planner change that moves any of it shows in the log and fails where a condition stops holding."""
import threading

import numpy as np
import pytest
import torch

import zly
import zly_model as zm
from batch_sweep_ref import (c2f_shape, carries_to_cv2, check_membership, count_launches, fused_block_names, pixel_tiles_per_wave, same_result,
                             same_slab, slab_key, table_ids, tail_box_levels)
from closed_loop_ref import check_closed_loop, check_head_decode, lds_resident_from_kernels
from oracle_lib import det_fields_equal

pytestmark = pytest.mark.gpu

CAP = 128
PROD_FLAGS = zly.FLAG_NO_HEAD_TENSOR | zly.FLAG_ASYNC_NMS


def _as_held(x):
    """what the bf16 front kernels hold for a preprocessed frame: bf16(u8 / 255)"""
    return torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()


class Sweep:
    """one FLAG_DUMP_LOGITS engine and max_batch distinct frames of the model's size, on the host and on the device"""

    def __init__(self, path, scale, w, h, max_batch, seed):
        self.path, self.w, self.h, self.max_batch = path, w, h, max_batch
        self.n_convs = len(zm.build_spec(scale).convs)
        self.host = zm.synth_frames(max_batch, w, h, seed=seed, rects=False)
        self.dev = torch.from_numpy(self.host).cuda()
        torch.cuda.synchronize()
        self.e = zly.Engine(path, model_w=w, model_h=h, max_batch=max_batch, max_dets=CAP, warmup_runs=0, flags=zly.FLAG_DUMP_LOGITS)
        self.slabs = {}

    def run(self, n):
        """zly_detect_device on the first n frames; the taps and the head tensor are those of this call until the next one"""
        self.e.detect_device(self.dev.data_ptr(), n, self.w, self.h)
        self.slabs[n] = self.e.read_slabs(n)
        return self.slabs[n]

    def slabs_at(self, n):
        return self.slabs[n] if n in self.slabs else self.run(n)

    def close(self):
        self.e.close()


@pytest.fixture(scope="module")
def sweep416(weights_path):
    s = Sweep(weights_path, "n", 416, 416, 64, seed=83)
    yield s
    s.close()


@pytest.fixture(scope="module")
def sweep352(weights_path):
    s = Sweep(weights_path, "n", 352, 288, 64, seed=84)
    yield s
    s.close()


@pytest.fixture(scope="module")
def sweep_s(tmp_path_factory):
    spec = zm.build_spec("s")
    p = str(tmp_path_factory.mktemp("batch_sweep") / "yolov8s_synth.zlyw")
    zm.write_zlyw(p, spec, zm.synth_weights(spec, seed=9))
    s = Sweep(p, "s", 352, 288, 32, seed=85)
    yield s
    s.close()


@pytest.fixture(scope="module")
def prod416(weights_path):
    e = zly.Engine(weights_path, max_batch=64, max_dets=CAP, warmup_runs=1, flags=PROD_FLAGS)
    yield e
    e.close()


def _closed_loop_case(sw, oracle, n):
    slabs = sw.run(n)
    ends = sorted({0, n - 1})
    lds = lds_resident_from_kernels(sw.e, n)
    x = _as_held(np.stack([oracle.preprocess(sw.host[i], sw.w, sw.h)[1] for i in ends]))
    assert len(check_closed_loop(sw.e, sw.path, ends, lds_resident=lds, first_input=x)) == sw.n_convs
    for i in ends:
        head = sw.e.head_tensor(i)
        check_head_decode(sw.e, head, i)
        want = oracle.postprocess(head, sw.w, sw.h)
        hdr, dets = slabs[i]
        assert int(hdr["n_kept"]) == len(want) and int(hdr["frame_tag"]) == i and det_fields_equal(dets, want[:CAP]), (n, i, int(hdr["n_kept"]), len(want))


# ---------------------------------------------------------------------------------------------------
# 1. per element against float64 at every batch size
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(1, 65))
def test_closed_loop_416(sweep416, oracle, n):
    _closed_loop_case(sweep416, oracle, n)


@pytest.mark.parametrize("n", range(1, 65))
def test_closed_loop_352x288(sweep352, oracle, n):
    _closed_loop_case(sweep352, oracle, n)


@pytest.mark.parametrize("n", range(1, 33))
def test_closed_loop_yolov8s_352x288(sweep_s, oracle, n):
    _closed_loop_case(sweep_s, oracle, n)


# ---------------------------------------------------------------------------------------------------
# 2. what the sweep reached, read off the engine's own launch tables
# ---------------------------------------------------------------------------------------------------
def test_coverage_is_recorded(sweep416, prod416):
    e = sweep416.e
    op_names = [o["name"] for o in e.ops()]
    tables = {n: e.op_kernels(n) for n in range(1, 65)}
    ids, n_tables = table_ids(tables)
    print(f"\n416 x 416, FLAG_DUMP_LOGITS: {n_tables} distinct launch tables over n = 1 .. 64;  n -> table id:")
    print("  " + " ".join(f"{n}:{ids[n]}" for n in range(1, 65)))
    blocks = fused_block_names(op_names, tables)
    assert len(blocks) == 4, sorted(blocks)                                 # model.2, the two halves of model.4, model.15
    for lead, by_n in sorted(blocks.items()):
        names = sorted(set(by_n.values()))
        shapes = sorted({c2f_shape(k)[2:] for k in names})
        print(f"  fused block at {lead}: fused at {len(by_n)} of 64 batch sizes, {len(names)} distinct kernel names, tiles " +
              " ".join(f"{a}x{b}" for a, b in shapes))
        assert len(names) >= 8, (lead, names)
    # conv B's results carried in registers to cv2: more than one pixel tile per wave under the DEFAULT plan at some n other than 64, never more than four
    carried = {}
    for n, kern in tables.items():
        for k in kern:
            if carries_to_cv2(k):
                t, nw = pixel_tiles_per_wave(k)
                assert t <= 4 * nw, (n, k)
                carried[n] = max(carried.get(n, 0), -(-t // nw))
    several = sorted(n for n, r in carried.items() if r > 1)
    print(f"  largest number of pixel tiles a wave carries to cv2: {max(carried.values())};  more than one at n = {several}")
    assert any(n != 64 for n in several), carried
    # both sides of each threshold
    for n in range(1, 65):
        assert count_launches(tables[n], "conv_igemm_multi_kernel") == (2 if n <= 4 else 0), (n, tables[n])
        assert count_launches(tables[n], "head_fused_kernel") == (3 if n >= 16 else 1), (n, tables[n])     # per-level tails on the side lanes
    # the production engine: the tail takes the box conv at some n (it switches on by itself), and it too has both sides of n >= 16.  The deferral of the NMS
    # itself (run_path, n >= 16 with FLAG_ASYNC_NMS) is no entry of the launch table; test_production_history_independence runs it on both sides.
    pnames = [o["name"] for o in prod416.ops()]
    ptables = {n: prod416.op_kernels(n) for n in range(1, 65)}
    pids, pn = table_ids(ptables)
    box_at = sorted(n for n in ptables if tail_box_levels(pnames, ptables[n]))
    print(f"production flags: {pn} distinct launch tables;  the tail computes the box conv at n = {box_at}")
    print("  " + " ".join(f"{n}:{pids[n]}" for n in range(1, 65)))
    assert box_at and min(box_at) > 4, box_at
    assert count_launches(ptables[15], "head_fused_kernel") == 1 and count_launches(ptables[16], "head_fused_kernel") == 3


# ---------------------------------------------------------------------------------------------------
# 3. the production flags give the dump engine's bytes at every n
# ---------------------------------------------------------------------------------------------------
def test_production_flags_give_the_dump_engines_slabs(sweep416, prod416):
    assert any(tail_box_levels([o["name"] for o in prod416.ops()], prod416.op_kernels(n)) for n in range(1, 65))
    bad, kept = [], 0
    for n in range(1, 65):
        want = sweep416.slabs_at(n)
        prod416.detect_device(sweep416.dev.data_ptr(), n, 416, 416)
        got = prod416.read_slabs(n)
        kept += sum(int(h["n_kept"]) for h, _ in want)
        bad += [(n, i, int(got[i][0]["n_kept"]), int(want[i][0]["n_kept"]), int(got[i][0]["n_candidates"]), int(want[i][0]["n_candidates"]))
                for i in range(n) if not same_slab(got[i], want[i])]
    assert kept > 0
    assert not bad, f"(n, frame, n_kept got / want, n_candidates got / want) of {len(bad)} differing slabs: {bad[:16]}"


# ---------------------------------------------------------------------------------------------------
# 4. history independence and position invariance
# ---------------------------------------------------------------------------------------------------
def _keys(e, dev, n, with_tag=True):
    e.detect_device(dev.data_ptr(), n, 416, 416)
    return [slab_key(h, d, with_tag) for h, d in e.read_slabs(n)]


def test_production_history_independence(sweep416, prod416):
    """every n on one engine in two different shuffled orders, read back after each call: the first visit captures the graph(s) of n, the second replays
    them after other neighbours; calls with deferred NMS (n >= 16, alternating candidate buffers) and joined ones interleave"""
    first_order = [int(v) for v in np.random.default_rng(1).permutation(np.arange(1, 65))]
    second_order = [int(v) for v in np.random.default_rng(2).permutation(np.arange(1, 65))]
    assert first_order != second_order
    for order in (first_order, second_order):                                # deferred and joined calls really alternate
        assert sum((a >= 16) != (b >= 16) for a, b in zip(order, order[1:])) >= 8, order
    first = {n: _keys(prod416, sweep416.dev, n) for n in first_order}
    second = {n: _keys(prod416, sweep416.dev, n) for n in second_order}
    bad = [(n, i) for n in range(1, 65) for i in range(n) if first[n][i] != second[n][i]]
    assert sum(k[0][0] for n in first for k in first[n]) > 0
    assert not bad, f"(n, frame) whose slab differs between the two visits: {bad[:32]}"
    # a third order, queued back to back with no host synchronisation in between, each call into a slab buffer of its own: the NMS of a deferred call
    # runs beside the next call whatever its batch size, and the two candidate buffers alternate across batch sizes
    third_order = [int(v) for v in np.random.default_rng(3).permutation(np.arange(1, 65))]
    e = prod416
    bufs = {n: torch.zeros(n * e.slab_bytes, dtype=torch.uint8, device="cuda") for n in third_order}
    torch.cuda.synchronize()
    for n in third_order:
        e.detect_device(sweep416.dev.data_ptr(), n, 416, 416, d_slabs_ptr=bufs[n].data_ptr())
    e.sync()
    third = {n: [slab_key(h, d) for h, d in zly.parse_slabs(bufs[n].cpu().numpy(), n, e.max_dets)] for n in third_order}
    bad = [(n, i) for n in range(1, 65) for i in range(n) if first[n][i] != third[n][i]]
    assert not bad, f"(n, frame) whose slab differs when the calls are queued back to back: {bad[:32]}"


@pytest.mark.parametrize("n", [3, 7, 17, 23, 49, 63])
def test_production_permutation_equivariance(sweep416, prod416, n):
    """3: merged Detect launches; 7; 17: just past the lanes / deferral threshold; 23 and 49: inside the two ranges in which a wave of model.4's back half
    carries two pixel tiles; 63: one frame short of the captured full batch"""
    want = _keys(prod416, sweep416.dev, n, with_tag=False)
    perm = np.random.default_rng(n).permutation(n)
    assert n < 2 or not np.array_equal(perm, np.arange(n))
    d2 = torch.from_numpy(sweep416.host[:n][perm]).cuda()
    torch.cuda.synchronize()
    got = _keys(prod416, d2, n, with_tag=False)
    assert len({k for k in want}) > 1                                        # the frames do differ in what they give
    bad = [i for i in range(n) if got[i] != want[perm[i]]]
    assert not bad, (n, bad)


# ---------------------------------------------------------------------------------------------------
# 5. the bf16 pipelined path at partial batches
# ---------------------------------------------------------------------------------------------------
def _mixed_frames():
    out = list(zm.synth_frames(6, 416, 416, seed=61, rects=False))
    out += [zm.synth_frames(1, 800, 600, seed=62, rects=False)[0], zm.synth_frames(1, 320, 240, seed=63)[0],
            zm.synth_frames(1, 64, 48, seed=64, rects=False)[0]]
    return [np.ascontiguousarray(f) for f in out]


def _table(e, frames, max_batch):
    """table[frame][n] = the frame's result inside a synchronous batch of n, the other positions filled with the remaining frames cyclically; a frame
    that occurs at several positions (or in several calls) of one n must give the same result at each"""
    nf = len(frames)
    table = {k: {} for k in range(nf)}
    for n in range(1, max_batch + 1):
        for start in range(0, nf, n):
            idx = [(start + j) % nf for j in range(n)]
            for k, res in zip(idx, e.detect_batch([frames[k] for k in idx], cap=CAP)):
                res = (res[0].copy(), res[1])
                assert same_result(table[k].setdefault(n, res), res), f"frame {k} depends on its position inside a batch of {n}"
    return table


def test_pipelined_partial_batches_bf16(weights_path):
    frames = _mixed_frames()
    ref = zly.Engine(weights_path, max_batch=24, max_dets=CAP, warmup_runs=1, flags=PROD_FLAGS)
    table = _table(ref, frames, 24)
    ref.close()
    assert all(sorted(t) == list(range(1, 25)) for t in table.values())
    with_dets = [k for k in table if table[k][1][1] > 0]
    assert len(with_dets) >= 6, {k: table[k][1][1] for k in table}
    for a in with_dets:                                                      # the table tells the frames apart
        for b in with_dets:
            assert a == b or not same_result(table[a][1], table[b][1]), (a, b)

    # the engine under test has never seen a synchronous call: it holds the graphs of batch 1 and batch 24 and launches every other size eagerly
    e = zly.Engine(weights_path, max_batch=24, max_dets=CAP, warmup_runs=1, flags=PROD_FLAGS)
    before = e.stats()
    per_thread, results, errors = 50, [], []
    tickets, lock, done, go = [], threading.Lock(), threading.Event(), threading.Barrier(4)

    def producer(tid):
        try:
            go.wait()
            for rep in range(per_thread):
                k = (rep + 2 * tid) % len(frames)
                t = e.submit(frames[k])
                with lock:
                    tickets.append((k, t))
        except Exception as exc:          # pragma: no cover
            errors.append(exc)

    # 200 frames against a ring of a few slots x 24: threads that only wait after submitting everything would dead-lock the ring, so a dedicated
    # consumer drains tickets as they are produced (the shape of the plugin's completion thread)
    def consumer(total):
        got = 0
        try:
            while got < total:
                with lock:
                    item = tickets.pop(0) if tickets else None
                if item is None:
                    if done.is_set() and not tickets:
                        break
                    continue
                k, t = item
                dets, n = e.wait(t, cap=CAP)
                results.append((k, (dets, n)))
                got += 1
        except Exception as exc:          # pragma: no cover
            errors.append(exc)

    ths = [threading.Thread(target=producer, args=(t,)) for t in range(4)]
    cons = threading.Thread(target=consumer, args=(4 * per_thread,))
    cons.start()
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    done.set()
    cons.join(timeout=120)
    after = e.stats()
    e.close()
    assert not errors, errors
    assert len(results) == 4 * per_thread
    matched = check_membership(results, table)
    d = {k: after[k] - before[k] for k in ("batches", "eager_batches", "graph_replays", "inference_errors", "inference_count")}
    sizes = sorted({m[0] for m in matched})
    print(f"\npipelined run: {len(results)} requests in {d['batches']} batches ({d['eager_batches']} eager, {d['graph_replays']} graph replays); "
          f"smallest matching batch size per ticket: {sizes}")
    assert d["inference_errors"] == 0 and d["inference_count"] == len(results), d
    assert d["eager_batches"] >= 1 and d["batches"] < len(results), d

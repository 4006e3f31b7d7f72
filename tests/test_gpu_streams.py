"""No result may depend on which stream is current.

On the default stream everything is ordered by accident: a launch that ignores its `stream` argument, a wrapper that
takes another stream than the caller's, a side stream that does not wait for the compute stream - none of them can fail
there.  Three tests make a side stream current:

  (a) every case of tests/_dirtycases.py and tests/_streamcases.py runs once inside `torch.cuda.stream(s)` with a
      recorder in front of the library (tests/_streams.py): every streamed entry point was given the current stream of
      the thread that called it, the test's thread gave `s` at least once and the null stream never, and the result is
      still the statement's.  The recorded names are checked against `_streamcases.REACHED`.
  (b) one split case per family behind a stall: the argument tensors hold decoys, the copy of the real inputs is queued
      behind a busy kernel on `s`, and the surface is called while the stream is provably still busy (`not s.query()`).
      Work that escaped to another stream ran on the decoy, or was overwritten afterwards.  Where the surface reads
      nothing back (`syncs` is empty) the stream must still be busy when the call returns, and more: an event recorded
      behind the stall and the copies must not have completed, since a stream is also "busy" with the call's own last
      kernel.  Where it does read back, the call has waited for the stream and nothing is asserted after it.
  (c) everything that owns a side stream or pinned staging, twice in a row with different contents behind a stall, with
      the default stream current and with a side stream current: both results equal their own statements.

The stall (100 ms) and its cap (500 ms) are conventions, not measured bounds: the `query()` assertions are the
condition, and a stall that is too short fails the test, it does not pass it.
"""
import threading

import numpy as np
import pytest
import torch

import _streamcases as C
import _streams as S

pytestmark = pytest.mark.gpu

ALL = C.all_cases()
_expected = {}


def _host(v):
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().numpy()
    return v if isinstance(v, bytes) else np.asarray(v)


# ----------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("cid", sorted(ALL))
def test_every_entry_point_is_given_the_current_stream(gpu_device, monkeypatch, cid):
    case = ALL[cid]
    if case.prepare is not None:
        case.prepare(gpu_device)
    with torch.cuda.device(gpu_device):
        torch.cuda.synchronize(gpu_device)
        s = torch.cuda.Stream(gpu_device)
        with monkeypatch.context() as mp:
            rec = S.install(mp)
            with torch.cuda.stream(s):
                got = case.run(gpu_device)
            s.synchronize()
        torch.cuda.synchronize(gpu_device)
        got = {name: _host(v) for name, v in got.items()}
    me = threading.get_ident()
    print(f"{cid}: {len(rec.calls)} streamed calls, {len({c.thread for c in rec.calls})} thread(s): {sorted(rec.names())}")
    wrong = [c for c in rec.calls if c.handle != c.current]
    assert not wrong, f"{cid}: calls that were not given their thread's current stream: {wrong[:5]}"
    mine = [c for c in rec.calls if c.thread == me]
    assert any(c.handle == s.cuda_stream for c in mine), f"{cid}: no call of this thread was given the stream that is current"
    assert not [c for c in mine if c.handle == 0], f"{cid}: calls on the null stream: {sorted({c.name for c in mine if c.handle == 0})}"
    claimed = {name for name, entry in C.REACHED.items() if isinstance(entry, tuple) and cid in entry}
    assert claimed <= rec.names(), f"{cid}: REACHED says this case calls {sorted(claimed - rec.names())}; it called {sorted(rec.names())}"
    if cid not in _expected:
        _expected[cid] = case.expected()
    case.compare(got, _expected[cid])


# ----------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("sid", sorted(C.SPLITS))
def test_behind_a_stall_the_call_reads_what_the_stream_wrote(gpu_device, sid):
    sp = C.SPLITS[sid]
    real, decoy = sp.inputs(), sp.decoy()
    with torch.cuda.device(gpu_device):
        box = sp.prepare(gpu_device) if sp.prepare else None
        args = {k: torch.from_numpy(np.array(v)).to(gpu_device) for k, v in decoy.items()}
        beside = {k: torch.from_numpy(np.array(v)).to(gpu_device) for k, v in real.items()}
        print(f"{sid}: {S.describe_calibration(gpu_device)}, a stall of {S.STALL_MS:.0f} ms, syncs: {sp.syncs or 'no'}")
        torch.cuda.synchronize(gpu_device)
        s = torch.cuda.Stream(gpu_device)
        with torch.cuda.stream(s):
            S.stall(s, S.STALL_MS)
            for k in args:
                args[k].copy_(beside[k])
            queued = torch.cuda.Event()
            queued.record(s)                         # behind the stall and the copies: done only once the real inputs are in place
            assert not s.query(), "the stall was over before the call was made"
            got = sp.call(args, box)
            busy, ahead = not s.query(), not queued.query()
            print(f"{sid}: when the call returned the stream was {'busy' if busy else 'idle'} and the stall {'still running' if ahead else 'over'}")
            if not sp.syncs:
                assert busy, "the stream was idle when the call returned: nothing shows that the call ran ahead of it"
                assert ahead, "the stall was over when the call returned: the call waited for the stream, or the stall is too short"
        s.synchronize()
        got = {name: _host(v) for name, v in got.items()}
    if sid not in _expected:
        _expected[sid] = sp.expected(real)
    sp.compare(got, _expected[sid])


# ----------------------------------------------------------------------------------------------------------- (c)
def _twice(device, side, first, second, spare_bytes=0):
    """`first()` then `second()` behind a stall on the stream that is current: the default one, or a side stream.
    `spare_bytes`: a block of that size is allocated before the first call and let go between the two, so that the second
    call's first allocation of that size takes it and its later ones fall where the first call's did."""
    with torch.cuda.device(device):
        torch.cuda.synchronize(device)
        cur = torch.cuda.Stream(device) if side else torch.cuda.current_stream(device)
        with torch.cuda.stream(cur):
            spare = [torch.empty(spare_bytes, dtype=torch.uint8, device=device)] if spare_bytes else []
            S.stall(cur, S.STALL_MS)
            a = first()
            spare.clear()
            b = second()
        cur.synchronize()
        torch.cuda.synchronize(device)
    return a, b


CURRENT = pytest.mark.parametrize("side", [False, True], ids=["default_stream", "side_stream"])


@pytest.fixture(scope="module")
def i420_clips(tmp_path_factory):
    """Two clips of the shape of tests/test_gpu_i420_in.py's fixture (five 6 x 18 frames): their I420 bytes, their Y4M
    files written on the host, and the statement's RGB."""
    import _handoff_ref as F
    import _i420_in_ref as R
    from elvis_amd import handoff
    out = []
    for seed in (31, 32):
        frames = np.random.default_rng(seed).integers(0, 256, (5, 6, 18, 3), dtype=np.uint8)
        planes = F.rgb_to_i420(frames)
        path = str(tmp_path_factory.mktemp("streams") / f"clip{seed}.y4m")
        with open(path, "wb") as f:
            f.write(handoff.y4m_header(18, 6, 25.0))
            for p in planes:
                f.write(b"FRAME\n" + p.tobytes())
        out.append((planes.tobytes(), path, R.i420_to_rgb(planes, "rgb")))
    assert not np.array_equal(out[0][2], out[1][2])
    return out


@CURRENT
@pytest.mark.parametrize("chunk", [None, 1], ids=["one_slot", "two_slots"])
@pytest.mark.parametrize("source", ["bytes", "y4m"])
def test_handoff_twice_in_a_row(gpu_device, i420_clips, source, chunk, side):
    """`handoff._planes_to_clip` uploads on a copy stream of its own.  Before that stream waited for the compute stream, a
    call returned once its uploads were done, and the next call's uploads could overwrite a staging block that the first
    call's conversion, still queued behind the stall, had yet to read.  Measured on an MI355X against that code: two of
    these eight cases failed (bytes / one slot / default stream and y4m / one slot / side stream), each with 1607 of the
    first clip's 1620 bytes equal to the second clip's; which cases show it depends on where the allocator puts the
    blocks.  Without the spare block none did: the second call's clip, not its staging, took the block."""
    from elvis_amd import handoff
    (raw_a, path_a, want_a), (raw_b, path_b, want_b) = i420_clips
    if source == "bytes":
        load = lambda raw, path: handoff.load_yuv420p_device(raw, 18, 6, gpu_device, "rgb", chunk_frames=chunk)
    else:
        load = lambda raw, path: handoff.load_y4m_device(path, gpu_device, "rgb", chunk_frames=chunk)
    # The clip is allocated before the staging.  With a free block of the clip's size at hand the second call's clip goes
    # there, and its staging gets the very block the first call's staging had: the one its conversion may still have to read.
    a, b = _twice(gpu_device, side, lambda: load(raw_a, path_a), lambda: load(raw_b, path_b), spare_bytes=want_a.size)
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.array_equal(b, want_b), "the second clip"
    bad = a != want_a
    assert not bad.any(), f"the first clip: {int(bad.sum())} of {bad.size} bytes differ ({int((a == want_b)[bad].sum())} of them are the second clip's)"


@pytest.fixture(scope="module")
def surface_clips():
    """tests/test_gpu_surfaces.py's clip maker: (n, h, w, seed) -> a list of frames."""
    import importlib
    return importlib.import_module("test_gpu_surfaces")._frames


@CURRENT
def test_single4x_host_twice_in_a_row(gpu_device, surface_clips, side):
    """tests/test_gpu_surfaces.py::test_host_to_host_pipeline_equals_device_path's clip and a second one: the oracle is
    the resident path, run before the stall."""
    from elvis_amd import restore
    from elvis_amd.weights import tiny_config
    model = restore.get_sinsr_model(gpu_device, cfg=tiny_config())
    lv = np.random.default_rng(22).integers(0, 3, size=(5, 8, 12)).astype(np.int32)
    lv[3] = 0
    lh = torch.from_numpy(lv).pin_memory()
    gidx = [40 + i for i in range(5)]
    clips = [torch.from_numpy(np.stack(surface_clips(5, 64, 96, seed))).pin_memory() for seed in (21, 23)]
    wants = [restore.restore_clip_single4x_device(model, fh.to(gpu_device), lh.to(gpu_device), 8, gidx, batch=2).cpu() for fh in clips]
    assert not torch.equal(wants[0], wants[1])
    outs = [torch.zeros_like(fh).pin_memory() for fh in clips]
    _twice(gpu_device, side, lambda: restore.restore_clip_single4x_host(model, clips[0], lh, 8, gidx, outs[0], batch=2),
           lambda: restore.restore_clip_single4x_host(model, clips[1], lh, 8, gidx, outs[1], batch=2))
    assert torch.equal(outs[1], wants[1]), "the second clip"
    assert torch.equal(outs[0], wants[0]), "the first clip"


@CURRENT
@pytest.mark.parametrize("kind", ["blur", "dct"])
def test_slot_host_twice_in_a_row(gpu_device, surface_clips, kind, side):
    """tests/test_gpu_surfaces.py::test_slot_host_pipelines_equal_the_frames_level_drivers' clip and a second one: the
    oracle is the frames-level driver, run before the stall."""
    import elvis_amd as E
    from elvis_amd import restore
    bm = np.random.default_rng(32).integers(0, 4, size=(7, 8, 12)).astype(np.int32)
    bm[2] = 0
    bm[5] = np.minimum(bm[5], 1)
    fn, kw = (E.restore_frames_blur, dict(batch_size=2)) if kind == "blur" else (E.restore_frames_dct, {})
    clips = [surface_clips(7, 64, 96, seed) for seed in (31, 33)]
    wants = [np.stack(fn(frames, bm, 8, gpu_device, **kw)) for frames in clips]
    assert not np.array_equal(wants[0], wants[1])
    model = restore._get_restorer(kind, gpu_device, False)
    mh = torch.from_numpy(bm).pin_memory()
    pinned = [torch.from_numpy(np.stack(frames)).pin_memory() for frames in clips]
    outs = [torch.zeros_like(fh).pin_memory() for fh in pinned]
    _twice(gpu_device, side, lambda: restore.restore_clip_slot_host(kind, model, pinned[0], mh, 8, outs[0], batch_size=2, upload_chunk=3),
           lambda: restore.restore_clip_slot_host(kind, model, pinned[1], mh, 8, outs[1], batch_size=2, upload_chunk=3))
    assert np.array_equal(outs[1].numpy(), wants[1]), "the second clip"
    assert np.array_equal(outs[0].numpy(), wants[0]), "the first clip"


def _stats_tolerance(scores, err):
    """How far each statistic of `vmaf_stats` may move when score i moves by at most err[i]: the sum over the scores of
    the statistic's change under +-err[i], doubled for what is not linear."""
    from elvis_amd import vmaf
    base = vmaf.vmaf_stats(scores)
    total = {k: 0.0 for k in base}
    for i in range(len(scores)):
        worst = {k: 0.0 for k in base}
        for sign in (-1.0, 1.0):
            moved = list(scores)
            moved[i] += sign * float(err[i])
            for k, v in vmaf.vmaf_stats(moved).items():
                worst[k] = max(worst[k], abs(v - base[k]))
        for k in base:
            total[k] += worst[k]
    return {k: 2.0 * total[k] for k in base}


@pytest.fixture(scope="module")
def vmaf_files(tmp_path_factory):
    """Two pairs of 64 x 64 raw I420 clips of three frames (the chroma planes are never read) and the statement's
    statistics of each pair."""
    import _vmaf_ref as R
    from elvis_amd import vmaf
    d = tmp_path_factory.mktemp("streams_vmaf")
    out = []
    for k, n in enumerate((3, 3)):
        ref, dis = R.fixture(64, 64, n + k)
        ref, dis = ref[k:], dis[k:]
        paths = []
        for name, planes in (("ref", ref), ("dis", dis)):
            paths.append(str(d / f"{name}{k}.yuv"))
            with open(paths[-1], "wb") as f:
                for p in planes:
                    f.write(p.tobytes() + bytes([128]) * (64 * 64 // 2))
        scores = R.score(R.features(ref, dis), vmaf.make_vmaf_model(0))
        err = R.BAR * np.maximum(1.0, np.abs(scores))
        out.append((paths, vmaf.vmaf_stats(scores), _stats_tolerance([float(v) for v in scores], err)))
    assert out[0][1] != out[1][1]
    return out


@CURRENT
def test_calculate_vmaf_twice_in_a_row(gpu_device, vmaf_files, side):
    from elvis_amd import vmaf
    (paths_a, want_a, tol_a), (paths_b, want_b, tol_b) = vmaf_files
    a, b = _twice(gpu_device, side, lambda: vmaf.calculate_vmaf(*paths_a, 64, 64, 30.0, device=gpu_device, chunk_frames=1),
                  lambda: vmaf.calculate_vmaf(*paths_b, 64, 64, 30.0, device=gpu_device, chunk_frames=1))
    for got, want, tol, which in ((b, want_b, tol_b, "second"), (a, want_a, tol_a, "first")):
        for k in want:
            assert abs(got[k] - want[k]) <= tol[k], f"the {which} pair's {k}: {got[k]} against the statement's {want[k]} (+- {tol[k]:.3g})"

"""The ledger of the stream tests, on the CPU: every streamed entry point of include/elvis_amd.h takes its stream last and
is bound that way, every launch, copy and fill in elvis_amd/csrc goes to the caller's stream (and the scanner that says
so reports a launch that does not), the recorder records what it is given, tests/_streamcases.py accounts for every
streamed entry point, and every split case's decoy would be noticed."""
import ctypes
import threading

import numpy as np
import pytest

import _streamcases as C
import _streams as S
from elvis_amd import _lib


# ----------------------------------------------------------------------------------------------------------- the header
def test_every_streamed_prototype_takes_its_stream_last_and_is_bound_so():
    protos = S.streamed_entry_points()
    text = S._uncomment(S.HEADER.read_text())
    assert len(protos) == text.count("elvis_stream_t") - 1 >= 90           # the header's own count; one mention is the typedef
    for p in protos:
        assert p.stream == len(p.params) - 1, f"{p.name}: the stream is parameter {p.stream} of {len(p.params)}"
        assert p.params[p.stream] == ("elvis_stream_t", "stream"), p
        bound = _lib.SIGNATURES.get(p.name)
        assert bound is not None and len(bound) == len(p.params), f"{p.name}: not bound with {len(p.params)} arguments"
        assert bound[p.stream] is ctypes.c_void_p, f"{p.name}: argument {p.stream} is bound as {bound[p.stream]}, not as a pointer"
    assert len({p.name for p in protos}) == len(protos)


def test_a_prototype_that_cannot_be_read_is_an_error():
    good = "typedef void* elvis_stream_t;\nint elvis_a(const float* x, int n, elvis_stream_t stream);\nsize_t elvis_b(int n);\n"
    assert [(p.name, p.stream) for p in S.streamed_entry_points(good)] == [("elvis_a", 2)]
    for bad in (good + "int elvis_c(int (*fn)(int), elvis_stream_t stream);\n",          # a parameter the parser does not take
                good + "void elvis_d(int n, elvis_stream_t stream);\n",                  # another return type
                good + "int elvis_e(elvis_stream_t a, elvis_stream_t b);\n",             # two streams
                good + "int elvis_f(int, elvis_stream_t stream);\n"):                    # a parameter without a name
        with pytest.raises(ValueError):
            S.streamed_entry_points(bad)


# ----------------------------------------------------------------------------------------------------------- the launches
def test_every_launch_copy_and_fill_in_csrc_goes_to_the_callers_stream():
    found = S.scan_tree()
    bad = [f for f in found if f.problem]
    assert not bad, "\n".join(f"{f.path}:{f.line}: {f.api} on `{f.stream}`: {f.problem}" for f in bad)
    launches = [f for f in found if f.api == "hipLaunchKernelGGL"]
    total = sum(p.read_text().count("hipLaunchKernelGGL(") for p in S.csrc_files())
    assert len(launches) == total >= 150, (len(launches), total)            # every spelling in the sources was read
    assert {f.kind for f in found} <= {"cast", "parameter", "local"}
    assert {f.api for f in found} <= {"hipLaunchKernelGGL", "hipMemcpyAsync", "hipMemsetAsync"}
    assert any(f.api == "hipMemcpyAsync" and f.path.endswith("vq_index.hip") for f in found)


FUNCTION = """
namespace {{
__global__ void k(int* p) {{ *p = 1; }}
}}
extern "C" int elvis_x(int* p, elvis_stream_t stream) {{
    {body}
    return 0;
}}
"""


def _scan(body, function=FUNCTION):
    return S.scan_source(function.format(body=body))


def test_the_scanner_takes_the_three_spellings_of_the_callers_stream():
    assert [f.kind for f in _scan("hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, (hipStream_t)stream, p);")] == ["cast"]
    assert [f.kind for f in _scan("hipStream_t s = (hipStream_t)stream;\n    hipLaunchKernelGGL((k2<a, b>), dim3(g(1, 2)), dim3(64), 0, s, p);")] == ["local"]
    helper = "static int launch(int* p, hipStream_t st) {{\n    {body}\n    return 0;\n}}\n"
    assert [f.kind for f in _scan("hipLaunchKernelGGL(k, dim3(1), dim3(64), q->bytes, st, p);", helper)] == ["parameter"]
    got = _scan("hipStream_t s = (hipStream_t)stream;\n    hipMemsetAsync(p, 0, 4, s);\n    hipMemcpyAsync(p, p, 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);")
    assert [(f.api, f.kind) for f in got] == [("hipMemsetAsync", "local"), ("hipMemcpyAsync", "cast")]
    # a launch inside a macro of the function, its kernel name in a string beside it
    macro = '#define LAUNCH(C) \\\n    hipLaunchKernelGGL(k<C>, dim3(1), dim3(64), 0, (hipStream_t)stream, p); \\\n    note("k<" #C ">")\n    LAUNCH(1);'
    assert [f.kind for f in _scan(macro)] == ["cast"]


@pytest.mark.parametrize("body,what", [
    ("hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, p);", "`0`"),
    ("hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, nullptr, p);", "`nullptr`"),
    ("hipStream_t s = hipStreamDefault;\n    hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, s, p);", "hipStreamDefault"),
    ("hipStream_t s = (hipStream_t)stream;\n    s = 0;\n    hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, s, p);", "assigned again"),
    ("hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, other, p);", "`other`"),
    ("hipLaunchKernelGGL(k, dim3(1), dim3(64), 0);", "the stream is the fifth"),
    ("hipMemcpy(p, p, 4, hipMemcpyDeviceToDevice);", "hipMemcpy"),
    ("hipMemset(p, 0, 4);", "hipMemset"),
    ("hipMemcpyToSymbol(sym, p, 4);", "hipMemcpyToSymbol"),
    ("hipMemcpyAsync(p, p, 4, hipMemcpyDeviceToDevice, 0);", "`0`"),
    ("hipMemsetAsync(p, 0, 4, nullptr);", "`nullptr`"),
    ("hipDeviceSynchronize();", "hipDeviceSynchronize"),
    ("k<<<1, 64, 0, (hipStream_t)stream>>>(p);", "<<<"),
    ("hipLaunchKernel((void*)k, dim3(1), dim3(64), args, 0, (hipStream_t)stream);", "hipLaunchKernel "),
    ("hipModuleLaunchKernel(f, 1, 1, 1, 64, 1, 1, 0, (hipStream_t)stream, args, nullptr);", "hipModuleLaunchKernel"),
])
def test_the_scanner_reports_a_defect(body, what):
    bad = [f for f in _scan(body) if f.problem]
    assert len(bad) == 1 and what in bad[0].problem + " ", (what, bad)


def test_the_scanner_reports_a_launch_whose_stream_is_not_the_functions_own():
    # `stream` that is no parameter of the enclosing function, and a launch outside every function
    orphan = "static int f(int* p) {{\n    {body}\n    return 0;\n}}\n"
    assert [bool(f.problem) for f in _scan("hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, (hipStream_t)stream, p);", orphan)] == [True]
    assert [bool(f.problem) for f in S.scan_source("hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, (hipStream_t)stream, p);\n")] == [True]
    with pytest.raises(ValueError):
        S.scan_source("int f() {\n")


# ----------------------------------------------------------------------------------------------------------- the recorder
class _Fn:
    def __init__(self, name):
        self.name, self.argtypes, self.restype, self.seen = name, ["given"], int, []

    def __call__(self, *args):
        self.seen.append(args)
        return 7


class _Handle:
    def __init__(self):
        self.elvis_a, self.elvis_b = _Fn("elvis_a"), _Fn("elvis_b")
        self.plain = "an attribute"


def test_the_recorder_records_streamed_calls_and_passes_everything_else_through():
    handle, current = _Handle(), threading.local()
    protos = S.streamed_entry_points("typedef void* elvis_stream_t;\nint elvis_a(const float* x, int n, elvis_stream_t stream);\nsize_t elvis_b(int n);\n")
    rec = S.Recorder(handle, protos, current=lambda: getattr(current, "stream", 0))
    assert rec.plain == "an attribute" and rec.elvis_b is handle.elvis_b and rec.elvis_b(3) == 7 and rec.calls == []
    current.stream = 11
    assert rec.elvis_a(1, 2, 11) == 7 and rec.elvis_a(1, 2, None) == 7 and rec.elvis_a(1, 2, ctypes.c_void_p(5)) == 7
    assert handle.elvis_a.seen[0] == (1, 2, 11) and handle.elvis_a.seen[1] == (1, 2, None)           # forwarded as given
    me = threading.get_ident()
    assert rec.calls == [S.Call("elvis_a", 11, 11, me), S.Call("elvis_a", 0, 11, me), S.Call("elvis_a", 5, 11, me)]
    # restype and argtypes read and write through to the function
    assert rec.elvis_a.argtypes == ["given"] and rec.elvis_a.restype is int
    rec.elvis_a.restype = ctypes.c_size_t
    assert handle.elvis_a.restype is ctypes.c_size_t
    rec.other = 3
    assert handle.other == 3
    with pytest.raises(AttributeError):
        rec.missing
    with pytest.raises(TypeError):
        rec.elvis_a(1, 2)                                                     # no stream argument at all

    def worker():
        current.stream = 23                                                   # this thread's own current stream
        rec.elvis_a(0, 0, 23)
        rec.elvis_a(0, 0, 11)                                                 # the other thread's stream: a defect the record shows

    t = threading.Thread(target=worker)
    t.start()
    t.join()
    late = rec.calls[3:]
    assert [(c.handle, c.current) for c in late] == [(23, 23), (11, 23)] and late[0].thread == t.ident != me
    assert rec.names() == {"elvis_a"}


def test_the_recorder_stands_in_for_the_loaded_library(monkeypatch, built_lib):
    real = _lib.lib()
    with monkeypatch.context() as mp:
        rec = S.Recorder(real, current=lambda: 0)
        mp.setattr(_lib, "_lib", rec)
        assert _lib.lib() is rec and _lib.lib().elvis_abi_version() == 1
        assert _lib.lib().elvis_vq_index_bytes.restype is ctypes.c_size_t
        # argument validation happens before the device is touched: ELVIS_E_INVALID, recorded with the null stream it was given
        assert _lib.lib().elvis_area_downscale_u8(1, 2, 1, 10, 16, 3, 4, 0, None) == -1
        assert [(c.name, c.handle) for c in rec.calls] == [("elvis_area_downscale_u8", 0)]
    assert _lib.lib() is real


def test_the_stall_refuses_more_than_its_cap():
    for ms in (0, -1, S.STALL_CAP_MS + 1):
        with pytest.raises(ValueError):
            S.stall(None, ms)
    assert 0 < S.STALL_MS <= S.STALL_CAP_MS == 500.0


# ----------------------------------------------------------------------------------------------------------- REACHED
def test_reached_accounts_for_every_streamed_entry_point():
    names = {p.name for p in S.streamed_entry_points()}
    missing, stale = sorted(names - set(C.REACHED)), sorted(set(C.REACHED) - names)
    assert not missing, f"streamed entry points tests/_streamcases.py REACHED does not list: {missing}"
    assert not stale, f"REACHED entries that are no streamed entry point of the header: {stale}"
    cases = C.all_cases()
    for name, entry in C.REACHED.items():
        if isinstance(entry, str):
            assert len(entry) >= 30, f"{name}: a reason of at least 30 characters"
        else:
            assert isinstance(entry, tuple) and entry and all(cid in cases for cid in entry), f"{name}: {entry}"


def test_the_cases_cover_the_dirty_table_and_every_family():
    import _dirtycases as D
    assert set(D.CASES) <= set(C.all_cases()) and len(D.CASES) == 62
    assert len(C.all_cases()) == len(D.CASES) + len(C.CASES)
    assert {c.family for c in D.CASES.values()} | {"jpeg_write", "resize", "vq_index", "gn_fused"} == set(C.FAMILIES)
    assert sorted(s.family for s in C.SPLITS.values()) == sorted(C.FAMILIES)                # one split case per family
    for cid in ("jpeg_write_restart_37x53_420", "jpeg_write_roi_37x53_420", "jpeg_write_opt_37x53_420", "png_write_rle_17x63",
                "split_jpeg_write_37x53_420", "split_resize_7x10", "split_vq_index_p257", "split_gn_fused_c64_t7"):
        assert cid in C.CASES, cid
    for s in C.SPLITS.values():
        assert isinstance(s.syncs, str) and (not s.syncs or len(s.syncs) >= 20), s.id


# ----------------------------------------------------------------------------------------------------------- the decoys
def _as_array(v):
    return np.frombuffer(v, np.uint8) if isinstance(v, bytes) else np.asarray(v)


@pytest.mark.parametrize("sid", sorted(C.SPLITS))
def test_a_kernel_that_read_the_decoy_would_be_noticed(sid):
    s = C.SPLITS[sid]
    real, decoy = s.inputs(), s.decoy()
    assert set(real) == set(decoy)
    for name, r in real.items():
        d = decoy[name]
        assert d.shape == r.shape and d.dtype == r.dtype and d.flags.c_contiguous, f"{sid}: the decoy of {name}"
        if r.dtype.kind in "iu":                                   # masks stay masks, maps and indices stay in range
            image = name in C.PIXELS and r.dtype == np.uint8          # every byte is a valid pixel
            assert image or set(np.unique(d)) <= set(np.unique(r)), f"{sid}: {name} leaves the input's values"
        else:
            assert np.isfinite(d).all(), f"{sid}: {name}"
    want_real, want_decoy = s.expected(real), s.expected(decoy)
    out_real, out_decoy = s.outputs(want_real), s.outputs(want_decoy)
    assert set(out_real) == set(out_decoy) and out_real
    bounds = s.bound(want_real) if s.bound else {}
    assert set(bounds) <= set(out_real) and (not s.bound or set(bounds) == set(out_real))
    for name in out_real:
        a, b = _as_array(out_real[name]), _as_array(out_decoy[name])
        if name in bounds:
            assert a.shape == b.shape
            far = np.abs(a.astype(np.float64) - b.astype(np.float64)) > bounds[name]
            assert far.mean() >= 0.5, f"{sid}: {name} differs by more than the bound at {far.mean():.2f} of the elements"
        else:
            assert a.shape != b.shape or (a != b).any(), f"{sid}: {name} is the same for the decoy"

"""The ledger of the dirty-allocation matrix, on the CPU: tests/_dirtycases.py lists every place the package asks for
uninitialised memory - no more, no fewer -, every entry points at something that exists, the cases stay small, the
poisoner does what tests/_dirty.py's table says, and a section that is cleared per call would be noticed if it were not."""
import ast
import pathlib
import struct

import numpy as np
import pytest
import torch

import _dirty
import _dirtycases as D

TESTS = pathlib.Path(__file__).resolve().parent


# ----------------------------------------------------------------------------------------------------------- the table
def test_the_ledger_lists_every_site_and_no_other():
    found = _dirty.sites()
    unlisted, stale = sorted(found - set(D.SITES)), sorted(set(D.SITES) - found)
    assert not unlisted, f"allocations the ledger does not list (add them to tests/_dirtycases.py SITES): {unlisted}"
    assert not stale, f"ledger entries whose allocation is gone (remove them from tests/_dirtycases.py SITES): {stale}"
    assert len(found) >= 80                        # the scan itself found the package
    counts = _dirty.site_counts()
    moved = {site: (n, D.SPELLINGS.get(site, 1)) for site, n in counts.items() if n != D.SPELLINGS.get(site, 1)}
    assert not moved, f"sites that spell their allocator another number of times than tests/_dirtycases.py SPELLINGS says (found, listed): {moved}"
    assert set(D.SPELLINGS) <= found and all(n > 1 for n in D.SPELLINGS.values())


SCANNED = '''
import torch
buf = torch.empty(1)
def plain(x):
    return torch.empty_like(x)
def conditional(zero):
    f = torch.zeros if zero else torch.empty
    return (torch.zeros if zero else torch.empty)(3), f
class K:
    def method(self, t):
        inner = lambda: t.new_empty(2)
        return [torch.empty(2) for _ in range(2)], inner
    @staticmethod
    def other():
        def nested():
            return torch.empty(1)
        return nested
def untouched(x):
    return torch.zeros(1), x.empty, empty(x), numpy.empty(3)
'''


def test_the_scan_sees_every_spelling_and_names_its_function():
    scan = _dirty._Scan("m")
    scan.visit(ast.parse(SCANNED))
    comp = "K.method.<locals>.<listcomp>" if hasattr(ast, "ListComp") and __import__("sys").version_info < (3, 12) else "K.method"
    assert scan.found == {("m", "<module>", "torch.empty"), ("m", "plain", "torch.empty_like"), ("m", "conditional", "torch.empty"),
                          ("m", "K.method.<locals>.<lambda>", "new_empty"), ("m", comp, "torch.empty"),
                          ("m", "K.other.<locals>.nested", "torch.empty")}
    # one allocation more, or one fewer, is another set: the ledger test above then names it
    more = _dirty._Scan("m")
    more.visit(ast.parse(SCANNED + "def added(n):\n    return torch.empty(n)\n"))
    assert more.found - scan.found == {("m", "added", "torch.empty")}
    fewer = _dirty._Scan("m")
    fewer.visit(ast.parse(SCANNED.replace("return torch.empty_like(x)", "return x.clone()")))
    assert scan.found - fewer.found == {("m", "plain", "torch.empty_like")}


def test_every_entry_is_one_of_the_three_kinds_and_points_at_something():
    for site, entry in D.SITES.items():
        assert isinstance(entry, tuple) and entry[0] in ("case", "prefilled", "host"), (site, entry)
        if entry[0] == "case":
            assert len(entry) in (2, 3) and entry[1] in D.CASES, f"{site}: no case {entry[1]!r}"
        elif entry[0] == "prefilled":
            assert len(entry) == 3 and "::" in entry[1] and entry[2], (site, entry)
        else:
            assert len(entry) == 2 and len(entry[1]) > 20, f"{site}: a host entry says why"
    # every integer-typed site says where its elements are written before they are read
    for site in D.INTEGER_SITES:
        assert site in D.SITES and len(D.INTEGER_SITES[site]) > 30, site
    claimed = {entry[1] for entry in D.SITES.values() if entry[0] == "case"}
    assert claimed <= set(D.CASES)


def _functions(tree):
    """The functions and classes of a file by name, and its module-level tables (a `RUN = {...}` of runners) by theirs."""
    out = {n.name: n for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.ClassDef))}
    for n in tree.body:
        if isinstance(n, ast.Assign) and isinstance(n.value, (ast.Dict, ast.Tuple, ast.List)):
            out.update({t.id: n.value for t in n.targets if isinstance(t, ast.Name)})
    return out


def _fills(node) -> bool:
    """Whether the code under `node` puts chosen contents into a tensor: `.fill_(`, `torch.full(` / `full_like(`, or an
    assignment to a slice or an index."""
    for n in ast.walk(node):
        if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr in ("fill_", "full", "full_like"):
            return True
        if isinstance(n, (ast.Assign, ast.AugAssign)):
            targets = n.targets if isinstance(n, ast.Assign) else [n.target]
            if any(isinstance(t, ast.Subscript) for t in targets):
                return True
    return False


def _reaches_a_fill(name, defs, seen=None) -> bool:
    """The named test, or a helper of its own file that it (transitively) names, fills a tensor."""
    seen = set() if seen is None else seen
    if name in seen or name not in defs:
        return False
    seen.add(name)
    node = defs[name]
    if _fills(node):
        return True
    used = {n.id for n in ast.walk(node) if isinstance(n, ast.Name)} | {n.attr for n in ast.walk(node) if isinstance(n, ast.Attribute)}
    return any(_reaches_a_fill(u, defs, seen) for u in sorted(used))


def test_every_prefilled_entry_names_a_test_that_fills_a_tensor():
    trees = {}
    for site, entry in D.SITES.items():
        if entry[0] != "prefilled":
            continue
        file, name = entry[1].split("::")
        path = TESTS / file
        assert path.is_file(), f"{site}: no test file {file}"
        if file not in trees:
            tree = ast.parse(path.read_text())
            defs = _functions(tree)
            for imp in (n for n in tree.body if isinstance(n, ast.ImportFrom) and n.module and (TESTS / f"{n.module}.py").is_file()):
                for k, v in _functions(ast.parse((TESTS / f"{imp.module}.py").read_text())).items():   # helpers imported from a sibling
                    defs.setdefault(k, v)
            trees[file] = (tree, defs)
        tree, defs = trees[file]
        tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
        assert name in tests, f"{site}: {file} has no test {name}"
        assert _reaches_a_fill(name, defs), f"{site}: {entry[1]} fills no tensor (no fill_, torch.full or slice assignment)"


def test_the_cases_stay_within_the_budget():
    for cid, case in D.CASES.items():
        n, h, w = case.clip
        assert h <= D.MAX_H and w <= D.MAX_W, f"{cid}: a {h} x {w} frame (at most {D.MAX_H} x {D.MAX_W})"
        if case.min_frames:
            # the surface takes no shorter clip: then exactly its minimum (FVMD's tracker, fvmd.MIN_REQUIRED_FRAMES)
            from elvis_amd import fvmd
            assert case.family == "fvmd" and n == case.min_frames == fvmd.MIN_REQUIRED_FRAMES, cid
        else:
            assert n <= D.MAX_FRAMES, f"{cid}: {n} frames (at most {D.MAX_FRAMES})"
    assert len(D.CASES) == len(set(D.CASES))


# ----------------------------------------------------------------------------------------------------------- the poisoner
def _package_dtypes():
    """Every `dtype=torch.X` the package writes in one of the scanned calls."""
    out = set()
    for path in sorted(_dirty.PKG.glob("*.py")):
        for call in (n for n in ast.walk(ast.parse(path.read_text())) if isinstance(n, ast.Call)):
            f = call.func
            if isinstance(f, ast.Attribute) and f.attr in ("empty", "empty_like", "new_empty"):
                for kw in call.keywords:
                    if kw.arg == "dtype" and isinstance(kw.value, ast.Attribute) and isinstance(kw.value.value, ast.Name) \
                            and kw.value.value.id == "torch":
                        out.add(getattr(torch, kw.value.attr))
    return out


@pytest.mark.parametrize("byte", _dirty.POISONS, ids=lambda b: f"0x{b:02X}")
def test_the_poisoner_fills_every_dtype_as_its_table_says(monkeypatch, byte):
    table = _dirty.READS_AS[byte]
    assert _package_dtypes() | {torch.float16, torch.float32, torch.float64, torch.int32, torch.uint8} <= set(table)
    # the table against the issue's own figures
    if byte == 0xFF:
        assert all(table[d] is None for d in (torch.float16, torch.float32, torch.float64))
        assert table[torch.int32] == -1 and table[torch.int8] == -1 and table[torch.uint8] == 255
    else:
        assert table[torch.float16] is None and 3.3e38 < table[torch.float32] < 3.5e38 and 1.3e306 < table[torch.float64] < 1.5e306
        assert table[torch.int32] == 2139062143 and table[torch.uint8] == 127
    assert struct.unpack("<d", bytes([0xA5]) * 8)[0] > -1e-100                     # why not 0xA5: it vanishes in any sum
    real = torch.empty
    with monkeypatch.context() as mp:
        seen = _dirty.poison(mp, byte)
        like = real(5, dtype=torch.float32)
        for dtype, want in table.items():
            made = [torch.empty((3, 2), dtype=dtype), torch.empty((), dtype=dtype), torch.empty_like(like, dtype=dtype),
                    like.new_empty((2,), dtype=dtype), (torch.zeros if False else torch.empty)(4, dtype=dtype)]
            for t in made:
                assert t.dtype == dtype and t.numel() > 0
                vals = t.reshape(-1)
                if want is None:
                    assert bool(torch.isnan(vals).all()), (dtype, byte)
                else:
                    assert vals.tolist() == [want] * vals.numel(), (dtype, byte, vals.tolist()[:2], want)
        assert torch.empty((0, 4)).numel() == 0 and like.new_empty((0,)).numel() == 0
        me = "test_the_poisoner_fills_every_dtype_as_its_table_says"
        assert {(__name__, me, "torch.empty"), (__name__, me, "torch.empty_like"), (__name__, me, "new_empty")} <= seen
    assert torch.empty is real                                                          # undone with the test


def test_the_poisoner_names_the_callers_qualified_function(monkeypatch):
    class Holder:
        def method(self):
            return [torch.empty(1) for _ in range(1)], (lambda: torch.empty(1))()

    with monkeypatch.context() as mp:
        seen = _dirty.poison(mp, 0x7F)
        Holder().method()
    names = {s[1] for s in seen}
    base = "test_the_poisoner_names_the_callers_qualified_function.<locals>.Holder.method"
    assert base + ".<locals>.<lambda>" in names
    assert (base + ".<locals>.<listcomp>" in names) or (base in names)               # a comprehension is inlined from 3.12


# ----------------------------------------------------------------------------------------------------------- discrimination
# For the families with an integer statement: would the chosen case notice?  An OUTPUT element that no thread writes is
# noticed without further argument - the comparison is byte for byte and no byte equals both 0xFF and 0x7F.  What needs
# showing is the sections that are only correct from a cleared start; they are restated here through the statements' own
# hooks, starting from the poison word instead of zero.
def _poison_word(byte, fmt):
    return struct.unpack(fmt, bytes([byte]) * struct.calcsize(fmt))[0]


@pytest.mark.parametrize("byte", _dirty.POISONS, ids=lambda b: f"0x{b:02X}")
def test_segment_histogram_and_count_from_the_poison_give_another_answer(byte):
    """csrc/segment.hip clears sad .. shift per call.  `details=True` gives F; the threshold is Otsu's over the histogram
    of F, the fallback compares the count of set pixels: both restated from a start at the poison word."""
    import _segment_ref as R
    frames, order, kw = R.cases()["48x64_n5"]
    cfg = R.SegmentConfig(**kw)
    masks, det = R.segment(frames, order, cfg, details=True)
    word = _poison_word(byte, "<I")
    hist = (np.bincount(det["F"][1].ravel(), minlength=256).astype(np.uint64) + word) % (1 << 32)
    assert R.otsu(hist) != int(det["thr"][1]), "the threshold of a histogram that starts at the poison"
    # the count: from 0xFF it is one short, which this frame's share does not notice - from 0x7F it is far above
    # max_share and the mask is dropped.  A section one poison leaves almost right is why there are two.
    pre = det["pre"][1]
    kept = lambda count: not (count == 0 or count * R.SHARE_DEN > R.share_num(cfg.max_share) * pre.size)
    assert kept(int(pre.sum()))
    assert not all(kept((int(pre.sum()) + _poison_word(b, "<I")) % (1 << 32)) for b in _dirty.POISONS)
    assert 0 < masks.mean() < 1
    # the flat clip: histogram and count stay at their cleared values, and that is what its all-ones answer rests on
    flat, order, kw = R.cases()["flat_40x52_n3"]
    fm, fd = R.segment(flat, order, R.SegmentConfig(**kw), details=True)
    assert not fd["sad"].any() and fm.all()
    # one frame: shift is read by the terms kernel without being computed; a poisoned shift is not (0, 0)
    assert _poison_word(byte, "<i") != 0 and not R.segment(*R.cases()["21x23_n1"][:2], details=True)[1]["shift"].any()


@pytest.mark.parametrize("byte", _dirty.POISONS, ids=lambda b: f"0x{b:02X}")
def test_inpaint_wave_counts_from_the_poison_give_another_launch_plan(byte):
    """csrc/inpaint.hip: workgroup 0 of the rows kernel clears the per-wave histogram.  The statement has no hook that
    takes a histogram (none is added); `wave_counts` states it, and the host reads the deepest wave off it."""
    import _inpaint_ref as R
    frames, masks = R.cases()["odd_random60"]
    want = R.wave_counts(masks)
    got = (want.astype(np.int64) + _poison_word(byte, "<i")).astype(np.int32)
    assert int(np.flatnonzero(got)[-1]) != int(np.flatnonzero(want)[-1]) and not np.array_equal(got, want)


@pytest.mark.parametrize("byte", _dirty.POISONS, ids=lambda b: f"0x{b:02X}")
def test_jpeg_coefficients_from_the_poison_give_other_samples(byte):
    """elvis_amd/jpeg.py clears the coefficient buffer per call (`_guarded(..., zero=True)`): the entropy kernel stores
    the coefficients a block codes and no others.  The statement's IDCT on a block whose uncoded coefficients hold the
    poison gives other samples."""
    import _jpeg_ref as R
    fc = next(f for f in R.files() if (f.h, f.w) == (17, 33))
    coef = R.decoded(fc.name).coef
    assert (coef == 0).any()
    dirty = np.where(coef == 0, _poison_word(byte, "<h"), coef)
    assert not np.array_equal(R.idct_blocks(dirty), R.idct_blocks(coef))


def test_the_families_without_a_cleared_section_say_so():
    """tfill, shrink / stretch and the PNG writer and reader keep nothing that is only correct from a cleared start in a
    fresh allocation: their reasons are in the table, and the table covers all six integer families."""
    assert set(D.DISCRIMINATION) == {"segment", "inpaint", "tfill", "shrink", "png", "jpeg"}
    assert all(len(v) > 40 for v in D.DISCRIMINATION.values())


# ----------------------------------------------------------------------------------------------------------- host packers
@pytest.mark.parametrize("net", ["rrdb", "srvgg"])
def test_the_host_packers_write_every_byte_of_their_image(net):
    """The RRDB and SRVGG weight images are packed on the host into `np.empty` (elvis_amd/_srnet.py), out of the
    poisoner's reach, so the property is checked here: the same image whatever the buffer held, for a conv whose real
    input channels (3, and 3 + 3 for RRDB's first layer) are fewer than the packed ones."""
    import ctypes as C
    from elvis_amd import _lib as L
    lib = L.lib()
    rng = np.random.default_rng(5)
    cin_real, cout_real = 3, 64
    w = np.ascontiguousarray(rng.standard_normal((cout_real, cin_real, 3, 3)).astype(np.float32))
    cin = 32
    cout = 64
    nbytes = getattr(lib, f"elvis_{net}_packed_weight_bytes")(cin, cout)
    assert nbytes > 0
    images = []
    for byte in (0x00,) + _dirty.POISONS:
        packed = np.full(nbytes // 2, byte * 0x0101, dtype=np.uint16)
        L.check(getattr(lib, f"elvis_{net}_pack_weights")(w.ctypes.data_as(C.c_void_p), cin_real, cout_real, cin, cout,
                                                           packed.ctypes.data_as(C.c_void_p)))
        images.append(packed.tobytes())
    assert images[0] == images[1] == images[2]
    assert any(images[0])

"""The library ledger: every kernel of the built library has a source, every source an owner, and every kernel of the
sources no area ledger owns a test that pins it (tests/_libledger.py says how and what a new kernel needs).  CPU only:
the library is cross-compiled, its symbols are read, and the test files are parsed, not run."""
import ast
import os
import re

import pytest

import _complexity_ref
import _gn_fused_model as GN
import _libledger as L
import _resize_ref
import _vq_grid_ref as VQ
from elvis_amd import _build

AREA_LEDGERS = sorted(set(L.OWNERS.values()) - {L.CLAIMS_OWNER})
CLAIMED_SOURCES = sorted(s for s, o in L.OWNERS.items() if o == L.CLAIMS_OWNER)


@pytest.fixture(scope="module")
def attributed(built_lib):
    return L.attribute(built_lib)


# ----------------------------------------------------------------------------- spelling
def test_spelling_reads_types_values_and_named_booleans_off_the_mangled_name():
    assert L.template_args("IDF16_EEvPKT_PS1_PixiiPKi") == ["half"] and L.template_args("IfEEvPKT_PS1_PixiiPKi") == ["float"]
    assert L.template_args("ILi16ELi3ELi1EEEvPKh") == ["16", "3", "1"] and L.template_args("PKhPhiiiii") == []
    assert L.template_args("IDF16_Li32ELi512ELi8ELb0ELi1ELb1EEEvNS_8ConvArgsE") == ["half", "32", "512", "8", "false", "1", "true"]
    assert L.spell("vq_grid_nearest_kernel", "IDF16_EEvPKT_PS1_PixiiPKi") == "vq_grid_nearest_kernel<half>"
    assert L.spell("resize_area_kernel", "ILb1ELb0EEEvPKhPhiiiiiNS_7AxisTabES4_iiiiiiif") == "resize_area_kernel<whole,lds>"
    assert L.spell("resize_area_kernel", "ILb0ELb1EEEvPKhPhiiiiiNS_7AxisTabES4_iiiiiiif") == "resize_area_kernel<frac,direct>"
    assert L.spell("rgb_to_i420_kernel", "ILb1EEEvPKhPhxiiii") == "rgb_to_i420_kernel<bgr>"
    assert L.spell("tfill_kernel", "ILi3EEEvPKhNS_8MaskViewEPhS4_NS_6ParamsE") == "tfill_kernel<3>"
    with pytest.raises(ValueError):
        L.template_args("IN3foo3barEEEvv")
    # the named booleans are the sources' own words: <WHOLE, DIRECT> and the notes of resize.hip, <BGR> and those of the hand-offs
    src = open(os.path.join(L.CSRC, "resize.hip")).read()
    assert "template <bool WHOLE, bool DIRECT>" in src and "ELVIS_AREA_LAUNCH(true, false);" in src
    assert set(_resize_ref.AREA_KERNELS.values()) | {_resize_ref.NEAREST_KERNEL} == set(L.CLAIMS["resize.hip"])
    for name, stem in (("i420_in.hip", "i420_to_rgb_kernel"), ("i420_in.hip", "i420_to_rgb_x16_kernel"), ("handoff.hip", "rgb_to_i420_kernel")):
        src = open(os.path.join(L.CSRC, name)).read()
        assert re.search(stem + r"<true>.*?\n.*?\n\s*elvis_note_launch\(\"" + stem + r"<bgr>\"\);", src), stem


# ----------------------------------------------------------------------------- enumeration and attribution
def test_every_kernel_symbol_has_exactly_one_source(attributed):
    kernels, orphans, doubles = attributed
    assert not orphans, f"kernels in the library that no file under elvis_amd/csrc declares: {orphans}"
    assert not doubles, f"__global__ stems declared by two sources: {doubles}"


def test_every_global_of_a_built_source_has_a_symbol(built_lib, attributed):
    kernels = attributed[0]
    have = {stem for stem, _ in L.stubs(built_lib)}
    built = set(_build.SOURCES)
    text = {f: open(os.path.join(L.CSRC, f)).read() for f in L.source_files()}
    # a header or .inc counts as built where a built source includes it
    for f, t in text.items():
        if f not in built and any(re.search(r'#include\s+"' + re.escape(f) + '"', text[s]) for s in text if s in built or s.endswith(".inc")):
            built.add(f)
    for f, stems in L.stems_by_source().items():
        assert f in built, f"{f} declares kernels {sorted(stems)} but no built source includes it"
        missing = sorted(stems - have)
        assert not missing, f"{f}: __global__ {missing} has no symbol in the library (never instantiated, or never launched)"
        assert kernels[f], f


def test_the_count_of_kernel_spellings(built_lib, attributed, capsys):
    kernels = attributed[0]
    per_owner, total = {}, 0
    for source in sorted(kernels):
        assert source in L.OWNERS, f"{source} holds kernels {sorted(kernels[source])} and has no owner in _libledger.OWNERS"
        count = len(L.spellings(built_lib, source))
        per_owner[L.OWNERS[source]] = per_owner.get(L.OWNERS[source], 0) + count
        total += count
    with capsys.disabled():
        print(f"\nlibrary ledger: {total} kernel spellings ({sum(len(v) for v in kernels.values())} instantiations): "
              + ", ".join(f"{o} {c}" for o, c in sorted(per_owner.items())))
    assert set(L.OWNERS) == set(kernels), sorted(set(L.OWNERS) ^ set(kernels))
    assert per_owner[L.CLAIMS_OWNER] == sum(len(v) for v in L.CLAIMS.values()) == 70
    assert total == 217          # 216 by _qualitycases.kernel_names alone, which cannot tell vq_grid_nearest_kernel's two types apart
    assert sum(len(v) for v in kernels.values()) == 313


# ----------------------------------------------------------------------------- owners
@pytest.mark.parametrize("ledger", AREA_LEDGERS)
def test_an_area_ledger_exists_and_names_its_sources(ledger):
    path = os.path.join(L.TESTS, ledger)
    assert os.path.exists(path), f"{ledger} owns sources in _libledger.OWNERS and does not exist"
    text = open(path).read()
    assert "built_lib" in text, f"{ledger} does not read the built library"
    by_source = L.stems_by_source()
    for source, owner in L.OWNERS.items():
        if owner == ledger:
            assert L.names_source(text, source, by_source[source]), f"{ledger} names neither {source} nor one of its kernels"


def test_the_claimed_sources_are_the_fourteen_without_an_area_ledger():
    assert CLAIMED_SOURCES == sorted(L.CLAIMS) and len(CLAIMED_SOURCES) == 14
    assert set(CLAIMED_SOURCES) <= set(_build.SOURCES)
    for ledger in AREA_LEDGERS:
        text = open(os.path.join(L.TESTS, ledger)).read()
        assert not any(s in text for s in CLAIMED_SOURCES if s != "segment.hip"), ledger


# ----------------------------------------------------------------------------- CLAIMS
@pytest.mark.parametrize("source", CLAIMED_SOURCES)
def test_claims_equal_the_librarys_kernels_in_both_directions(attributed, source):
    have, claimed = attributed[0][source], set(L.CLAIMS[source])
    assert not have - claimed, f"{source}: no test claims {sorted(have - claimed)} (add a noted, stage or sole claim to _libledger.CLAIMS)"
    assert not claimed - have, f"{source}: CLAIMS names {sorted(claimed - have)}, which the library does not hold"


# parametrisations whose ids come from a list in another module
ID_LISTS = {"test_gpu_complexity.py::test_matrix_within_the_bar": lambda: {c.kernel for c in _complexity_ref.MATRIX}}


def _id_is_parametrised(file_name, node, test, case_id):
    key = f"{file_name}::{test}"
    if key in ID_LISTS:
        return case_id in ID_LISTS[key]()
    src = open(os.path.join(L.TESTS, file_name)).read()
    decorators = " ".join(ast.get_source_segment(src, d) for d in node.decorator_list)
    return "parametrize" in decorators and all(re.search(r"[\"'\[( ,]" + re.escape(piece) + r"[\"'\]) ,]", decorators) for piece in case_id.split("-"))


@pytest.mark.parametrize("source", CLAIMED_SOURCES)
def test_every_claimed_test_exists_and_a_noted_claim_is_spelled_in_its_file(source):
    for kernel, (kind, entries, _) in L.CLAIMS[source].items():
        assert kind in ("noted", "stage", "sole") and entries, kernel
        for entry in entries:
            file_name, test, case_id = L.split_claim(entry)
            tests = L.tests_of(file_name)
            assert test in tests, f"{kernel}: {file_name} has no {test}"
            assert case_id is None or _id_is_parametrised(file_name, tests[test], test, case_id), f"{kernel}: {entry} is no case of {test}"
            text = open(os.path.join(L.TESTS, file_name)).read()
            assert "pytest.mark.gpu" in text, f"{kernel}: {file_name} is no GPU test file"
            if kind == "noted":
                assert "elvis_last_launch" in text or "_last_launch" in text, f"{kernel}: {file_name} never reads elvis_last_launch"
                for piece_file, piece in L.NOTED_PIECES.get(kernel, [(file_name, kernel)]):
                    assert piece in open(os.path.join(L.TESTS, piece_file)).read(), f"{kernel}: {piece_file} does not hold {piece!r}"
                # the source notes this very string, or formats it from the launcher's template parameters
                src = open(os.path.join(L.CSRC, source)).read()
                stem = kernel.split("<")[0]
                assert f'"{kernel}"' in src or re.search(r'ElvisKernelName name\("' + stem + r"<%d(,%d)*>\"", src), f"{kernel}: {source} never notes it"


def test_noted_pieces_belong_to_noted_claims():
    noted = {k for claims in L.CLAIMS.values() for k, (kind, _, _) in claims.items() if kind == "noted"}
    assert set(L.NOTED_PIECES) <= noted, sorted(set(L.NOTED_PIECES) - noted)
    # the complexity names are built by the reference's case list, which holds all nine
    assert {c.kernel for c in _complexity_ref.MATRIX} == set(L.CLAIMS["complexity.hip"])


# ----------------------------------------------------------------------------- the added cases stay small
def test_the_added_groupnorm_and_vq_cases_stay_small():
    assert GN.N_IMAGES <= 2 and max(t for _, _, t in GN.gpu_cases() + list(GN.CLAMP_CASES)) <= 769
    for case in VQ.CASES:
        cb, z = case.arrays()
        assert cb.shape[0] <= 20000 and z.shape[0] <= 1100, case.id

"""The library ledger (tests/test_library_ledger.py): every kernel of the built library, the source file it comes from,
and who answers for it.

Enumeration.  hipcc emits one host stub per kernel instantiation, `__device_stub__<stem>` with the kernel's own template
arguments and signature, so the stubs of the built library ARE the list of its kernels, whatever the sources say.  A stub
is attributed to the one file under elvis_amd/csrc (.hip, .inc or .h) whose text declares a `__global__` function of that
stem (`_glueref.kernel_stems`).

Spelling.  `_qualitycases.kernel_names` spells value template arguments (`tfill_kernel<3>`, `srvgg_conv3x3_kernel<64,
false>`) and drops type arguments, so `vq_grid_nearest_kernel<_Float16>` and `<float>` collapse into one name.  `spell`
reads the whole argument list off the mangled name and spells types as the sources' own elvis_note_launch strings do
(`DF16_` -> half, `f` -> float); boolean arguments may be given names (SPELL_BOOL: `resize_area_kernel<whole,lds>`).
The sources CLAIMS owns are spelled this way; a source owned by an area ledger keeps the helper's spelling, because that
ledger has a demangler of its own and its own lists, which are not copied here.

Owners.  OWNERS maps every source that holds a kernel to the test file that answers for it: one of the nine area ledgers,
or this module's CLAIMS.  CLAIMS gives, for every kernel spelling of its sources, the tests that pin it and how:

    noted   the test compares elvis_last_launch() with this spelling (the file holds the spelling, or the pieces its
            parametrisation builds it from: NOTED_PIECES)
    stage   the test compares a buffer that only this kernel writes
    sole    the entry point the test calls launches nothing else

A new kernel therefore needs three things before the suite passes again: a source that `_build.SOURCES` compiles, an
owner, and - where CLAIMS is the owner - a test of one of the three kinds.
"""
from __future__ import annotations

import ast
import os
import re
from typing import Dict, List, Optional, Set, Tuple

from _convref import elf_symbols
from _glueref import kernel_stems
from _qualitycases import kernel_names

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CSRC = os.path.join(ROOT, "elvis_amd", "csrc")

_STUB = re.compile(r"_Z(?:N12_GLOBAL__N_1)?(\d+)__device_stub__")
_TYPES = {"DF16_": "half", "f": "float", "d": "double", "h": "uint8_t", "i": "int"}
_ARG = re.compile(r"L([ib])(\d+)E|(DF16_|[fdhi])")

# boolean template arguments that the source's elvis_note_launch strings name instead of true / false
SPELL_BOOL = {"resize_area_kernel": (("frac", "whole"), ("lds", "direct"))}


# ============================================================================================ enumeration
def stubs(lib_path: str) -> List[Tuple[str, str]]:
    """(stem, the mangled remainder: template arguments and signature) of every kernel instantiation of the library."""
    out = []
    for sym in elf_symbols(lib_path):
        t = _STUB.match(sym)
        if not t:
            continue
        ln = int(t.group(1))
        at = t.end() - len("__device_stub__")
        out.append((sym[t.end():at + ln], sym[at + ln:]))
    return sorted(set(out))


def template_args(rest: str) -> List[str]:
    """`ILb1ELb0EEEvPKh...` -> ['true', 'false'], `IDF16_EEvPKT_...` -> ['half'], `ILi3EEEv..` -> ['3']; [] for a kernel
    that is no template.  Anything it cannot read is an error: the ledger must not guess a spelling."""
    if not rest.startswith("I"):
        return []
    args, pos = [], 1
    while rest[pos] != "E":
        t = _ARG.match(rest, pos)
        if not t:
            raise ValueError(f"template argument list not understood: {rest!r}")
        if t.group(3):
            args.append(_TYPES[t.group(3)])
        elif t.group(1) == "b":
            args.append(("false", "true")[int(t.group(2))])
        else:
            args.append(t.group(2))
        pos = t.end()
    return args


def spell(stem: str, rest: str) -> str:
    args = template_args(rest)
    names = SPELL_BOOL.get(stem)
    if names:
        args = [names[k][("false", "true").index(a)] for k, a in enumerate(args)]
    return f"{stem}<{','.join(args)}>" if args else stem


def source_files() -> List[str]:
    return sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".inc", ".h")))


def stems_by_source() -> Dict[str, Set[str]]:
    out = {f: kernel_stems(os.path.join(CSRC, f)) for f in source_files()}
    return {f: s for f, s in out.items() if s}


def attribute(lib_path: str):
    """(kernels: source -> the extended spellings of its instantiations, orphans: stubs no source declares, doubles: stems
    that two sources declare)."""
    by_source = stems_by_source()
    owner: Dict[str, List[str]] = {}
    for f, stems in by_source.items():
        for s in stems:
            owner.setdefault(s, []).append(f)
    kernels: Dict[str, Set[str]] = {f: set() for f in by_source}
    orphans = []
    for stem, rest in stubs(lib_path):
        if stem not in owner:
            orphans.append(stem)
        else:
            kernels[owner[stem][0]].add(spell(stem, rest))
    return kernels, sorted(set(orphans)), {s: f for s, f in owner.items() if len(f) > 1}


def spellings(lib_path: str, source: str) -> Set[str]:
    """What the ledger calls the kernels of one source: extended for a source of CLAIMS, the helper's otherwise."""
    if OWNERS[source] == CLAIMS_OWNER:
        return attribute(lib_path)[0][source]
    return kernel_names(lib_path, os.path.join(CSRC, source))


# ============================================================================================ owners
CLAIMS_OWNER = "test_library_ledger.py"
OWNERS = {
    "conv_kernels.inc": "test_conv_ledger.py", "conv_ws.inc": "test_conv_ledger.py", "conv_x3p.inc": "test_conv_ledger.py",
    "attn.hip": "test_model_kernels_ledger.py", "swin.hip": "test_model_kernels_ledger.py", "dcn.hip": "test_model_kernels_ledger.py",
    "norm.hip": "test_norm_misc_ledger.py", "misc.hip": "test_norm_misc_ledger.py",
    "glue.hip": "test_glue_ledger.py",
    "classical.hip": "test_block_ledger.py", "degrade.hip": "test_block_ledger.py", "shrink.hip": "test_block_ledger.py",
    "quality.hip": "test_quality_inpaint_ledger.py", "inpaint.hip": "test_quality_inpaint_ledger.py",
    "vmaf.hip": "test_vmaf_fvmd_ledger.py", "fvmd.hip": "test_vmaf_fvmd_ledger.py",
    "rrdb.hip": "test_sr_ledger.py", "srvgg.hip": "test_sr_ledger.py",
    "sr_enhance.hip": "test_enhance_ledger.py",
    **{s: CLAIMS_OWNER for s in ("png.hip", "png_read.hip", "jpeg_read.hip", "jpeg_write.hip", "segment.hip", "lpips.hip",
                                 "tfill.hip", "resize.hip", "i420_in.hip", "handoff.hip", "presley_degrade.hip",
                                 "complexity.hip", "vq_index.hip", "gn_fused.hip")},
}


def names_source(ledger_text: str, source: str, stems: Set[str]) -> bool:
    """An area ledger names a source by its file name or, where it works from the symbols alone (the conv and model
    ledgers), by the whole stem of one of the source's kernels."""
    return source in ledger_text or any(re.search(r"\b" + re.escape(s) + r"\b", ledger_text) for s in stems)


# ============================================================================================ test lookup
def tests_of(file_name: str) -> Dict[str, Optional[ast.AST]]:
    """The test functions of a test file, by name, from its syntax tree (the file is not imported)."""
    with open(os.path.join(TESTS, file_name)) as f:
        tree = ast.parse(f.read())
    return {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}


def split_claim(entry: str) -> Tuple[str, str, Optional[str]]:
    """`file::test` or `file::test[id]` -> (file, test, id or None)."""
    t = re.fullmatch(r"([\w.]+)::(\w+)(?:\[(.+)\])?", entry)
    if not t:
        raise ValueError(f"claim not understood: {entry!r}")
    return t.group(1), t.group(2), t.group(3)


# ============================================================================================ CLAIMS
# the boolean template arguments the sources' notes name (rgb / bgr)
SPELL_BOOL.update({k: (("rgb", "bgr"),) for k in ("i420_to_rgb_kernel", "i420_to_rgb_x16_kernel", "rgb_to_i420_kernel")})

_PNG, _RLE, _PNGR = "test_gpu_png.py", "test_gpu_png_rle.py", "test_gpu_png_read.py"
_JR, _JW, _SEG, _LP = "test_gpu_jpeg.py", "test_gpu_jpeg_write.py", "test_gpu_segment.py", "test_gpu_lpips.py"
_SEG_STAGES = f"{_SEG}::test_device_equals_the_statement_byte_for_byte"
_JW_BUFFERS = f"{_JW}::test_prefix_sums_stream_words_and_sizes_equal_what_the_statement_implies"

# source -> kernel spelling -> (kind, the tests that pin it, a note on what they compare)
CLAIMS = {
    "png.hip": {
        "png_stats_kernel": ("stage", [f"{_PNG}::test_types_statistics_and_guard_bytes"], "the filter types: no other kernel writes them"),
        "png_stats_rle_kernel": ("sole", [f"{_RLE}::test_types_statistics_and_guard_bytes"], "elvis_png_stats_rle called by the test itself"),
        "png_pack_kernel": ("stage", [f"{_PNG}::test_device_files_equal_the_statement"], "the IDAT data of the files"),
        "png_pack_rle_kernel": ("stage", [f"{_RLE}::test_device_files_equal_the_statement"], "the IDAT data of the files"),
        "png_crc_kernel": ("stage", [f"{_PNG}::test_device_files_equal_the_statement"], "every chunk's CRC field, also against zlib (_check_file)"),
    },
    "png_read.hip": {
        "png_gather_kernel": ("stage", [f"{_PNGR}::test_gather_concatenates_the_idat_payloads"], "the gathered zlib streams"),
        "png_crc_check_kernel": ("stage", [f"{_PNGR}::test_decode_uploads_off_a_dword", f"{_PNGR}::test_malformed_files_in_a_batch_with_good_frames"],
                                 "the chunks' status words: a frame's code E_CRC, and 0 for the good ones"),
        "png_inflate_kernel": ("sole", [f"{_PNGR}::test_inflate_every_stream_equals_zlib"], "png._inflate_clip is elvis_png_inflate alone"),
        "png_unfilter_kernel<1,1>": ("stage", [f"{_PNGR}::test_decode_gray_files_to_one_channel"], "the frames, gray files to one channel"),
        "png_unfilter_kernel<1,3>": ("stage", [f"{_PNGR}::test_decode_every_file_equals_pil"], "the frames, colour type 0 replicated"),
        "png_unfilter_kernel<3,3>": ("stage", [f"{_PNGR}::test_decode_every_file_equals_pil"], "the frames, colour type 2"),
        "png_unfilter_kernel<4,3>": ("stage", [f"{_PNGR}::test_decode_every_file_equals_pil"], "the frames, colour type 6 without alpha"),
    },
    "jpeg_read.hip": {
        "jpeg_tables_kernel": ("stage", [f"{_JR}::test_derived_code_tables_equal_their_statement"], "the derived code tables"),
        "jpeg_entropy_kernel": ("stage", [f"{_JR}::test_decode_every_file_equals_the_statement_and_pil"], "coef_buf and the segments' status words"),
        "jpeg_idct_kernel": ("stage", [f"{_JR}::test_decode_every_file_equals_the_statement_and_pil"], "plane_buf (_check_clip)"),
        "jpeg_colour_kernel<1>": ("stage", [f"{_JR}::test_decode_gray_files_to_one_channel"], "the frames"),
        "jpeg_colour_kernel<3>": ("stage", [f"{_JR}::test_decode_every_file_equals_the_statement_and_pil"], "the frames"),
    },
    "jpeg_write.hip": {
        "jpeg_fdct_kernel": ("stage", [f"{_JW}::test_device_bytes_equal_the_statement_and_pil"], "coef_buf"),
        "jpeg_bits_kernel": ("stage", [_JW_BUFFERS], "bits_buf: the differences of the offsets are its lengths"),
        "jpeg_scan_kernel": ("stage", [_JW_BUFFERS], "bits_buf and ffc_buf: exclusive prefix sums and totals"),
        "jpeg_clear_kernel": ("stage", [_JW_BUFFERS], "words_buf from 0xFF: the zero bytes up to the dword, and every bit the pack ORs into"),
        "jpeg_pack_kernel": ("stage", [_JW_BUFFERS], "words_buf: the unstuffed stream"),
        "jpeg_ff_kernel": ("stage", [_JW_BUFFERS], "ffc_buf: the FF bytes of every 1024-byte chunk"),
        "jpeg_sizes_kernel": ("stage", [_JW_BUFFERS], "sizes_buf"),
        "jpeg_stuff_kernel": ("stage", [f"{_JW}::test_device_bytes_equal_the_statement_and_pil"], "the finished scans"),
    },
    "segment.hip": {
        "seg_reduce_kernel<1>": ("stage", [_SEG_STAGES], "details red, one-channel cases"),
        "seg_reduce_kernel<3>": ("stage", [_SEG_STAGES], "details red"),
        "seg_strips_kernel": ("stage", [f"{_SEG}::test_strip_means_and_votes_equal_the_statement"], "details means"),
        "seg_sad_kernel": ("stage", [_SEG_STAGES], "details sad"),
        "seg_pick_kernel": ("stage", [_SEG_STAGES], "details shift"),
        "seg_terms_kernel": ("stage", [_SEG_STAGES], "details M, S"),
        "seg_fuse_kernel": ("stage", [_SEG_STAGES], "details Mn, Sn, F"),
        "seg_threshold_kernel": ("stage", [_SEG_STAGES], "details thr"),
        "seg_morph_kernel": ("stage", [_SEG_STAGES], "details pre"),
        "seg_vote_kernel": ("stage", [f"{_SEG}::test_strip_means_and_votes_equal_the_statement"], "details voted, count"),
        "seg_upsample_kernel": ("noted", [_SEG_STAGES], "and the masks"),
    },
    "lpips.hip": {
        "lpips_stem_kernel<0>": ("noted", [f"{_LP}::test_stem_within_the_conv_error_model[rgb]"], ""),
        "lpips_stem_kernel<1>": ("noted", [f"{_LP}::test_stem_within_the_conv_error_model[bgr]"], ""),
        "lpips_conv5_kernel": ("noted", [f"{_LP}::test_conv5_within_the_conv_error_model"], ""),
        "lpips_maxpool_kernel": ("noted", [f"{_LP}::test_maxpool_is_bit_exact"], ""),
        "lpips_distance_kernel": ("stage", [f"{_LP}::test_distance_partials_are_the_distance_kernels_own_output"], "the workspace of partial sums"),
        "lpips_finish_kernel": ("noted", [f"{_LP}::test_distance_per_tap"], ""),
    },
    "tfill.hip": {f"tfill_kernel<{c}>": ("noted", ["test_gpu_tfill.py::test_device_equals_the_numpy_statement"], "") for c in (1, 3)},
    "resize.hip": {
        **{f"resize_area_kernel<{a},{b}>": ("noted", ["test_gpu_resize.py::test_area_resize_is_the_statement_bit_for_bit"], "")
           for a in ("whole", "frac") for b in ("lds", "direct")},
        "resize_nearest_kernel": ("noted", ["test_gpu_resize.py::test_nearest_resize_is_the_statement_and_the_hosts"], ""),
    },
    "i420_in.hip": {
        **{f"i420_to_rgb_kernel<{o}>": ("noted", [f"test_gpu_i420_in.py::test_shape_matrix[{o}]"], "") for o in ("rgb", "bgr")},
        **{f"i420_to_rgb_x16_kernel<{o}>": ("noted", [f"test_gpu_i420_in.py::test_sixteen_pixel_strips[{o}]"], "") for o in ("rgb", "bgr")},
    },
    "handoff.hip": {
        "rgb_to_i420_kernel<bgr>": ("noted", ["test_gpu_handoff.py::test_errors_come_before_any_launch"], ""),
        "rgb_to_i420_kernel<rgb>": ("noted", ["test_gpu_i420_in.py::test_out_and_errors_come_before_any_launch"], ""),
    },
    "presley_degrade.hip": {
        "degrade_scale_kernel": ("noted", ["test_gpu_presley_degrade.py::test_degrade_scale_device", "test_gpu_presley_degrade.py::test_two_channels_through_both_kernels"], ""),
        "degrade_gaussian_fx_kernel": ("noted", ["test_gpu_presley_degrade.py::test_degrade_gaussian_fx_device", "test_gpu_presley_degrade.py::test_two_channels_through_both_kernels"], ""),
    },
    "complexity.hip": {f"block_complexity_kernel<{b},{c},{o}>": ("noted", [f"test_gpu_complexity.py::test_matrix_within_the_bar[block_complexity_kernel<{b},{c},{o}>]"], "")
                       for b in (8, 16, 32) for c, o in ((1, 0), (3, 0), (3, 1))},
    "vq_index.hip": {f"vq_grid_nearest_kernel<{t}>": ("noted", [f"test_gpu_vq_indexed.py::test_the_cases_of_the_host_model[{d}]"], "")
                     for t, d in (("half", "f16"), ("float", "f32"))},
    "gn_fused.hip": {f"gn_partials_affine_kernel<{rl}>": ("noted", ["test_gpu_gn_fused.py::test_new_spans_equal_the_model_and_the_two_launches"], "")
                     for rl in (4, 8)},
}

# Where a test builds the note's spelling instead of holding it: (file, the text that builds it), all of which must be
# in that file.  A spelling without an entry must stand in its test file as it is.
NOTED_PIECES = {
    **{f"lpips_stem_kernel<{o}>": [(_LP, "f\"lpips_stem_kernel<{int(order == 'bgr')}>\"")] for o in (0, 1)},
    **{f"tfill_kernel<{c}>": [("test_gpu_tfill.py", 'f"tfill_kernel<{frames.shape[3]}>"')] for c in (1, 3)},
    **{k: [("_resize_ref.py", f'"{k}"'), ("test_gpu_resize.py", "assert _launched() == R.area_kernel(hs, ws, hd, wd, c)")]
       for k in CLAIMS["resize.hip"] if k.startswith("resize_area")},
    "resize_nearest_kernel": [("_resize_ref.py", 'NEAREST_KERNEL = "resize_nearest_kernel"'), ("test_gpu_resize.py", "assert _launched() == R.NEAREST_KERNEL")],
    **{f"i420_to_rgb_kernel<{o}>": [("test_gpu_i420_in.py", 'f"i420_to_rgb_kernel<{order}>"')] for o in ("rgb", "bgr")},
    **{f"i420_to_rgb_x16_kernel<{o}>": [("test_gpu_i420_in.py", '"i420_to_rgb_x16_kernel"'), ("test_gpu_i420_in.py", 'f"{kernel}<{order}>"')]
       for o in ("rgb", "bgr")},
    **{k: [("_complexity_ref.py", "f\"block_complexity_kernel<{self.block},{self.shape[3]},{int(self.order == 'bgr')}>\""),
           ("test_gpu_complexity.py", "assert _lib.lib().elvis_last_launch().decode() == kernel")] for k in CLAIMS["complexity.hip"]},
    **{f"vq_grid_nearest_kernel<{t}>": [("test_gpu_vq_indexed.py", "f\"vq_grid_nearest_kernel<{'half' if dt == 'f16' else 'float'}>\"")]
       for t in ("half", "float")},
    **{f"gn_partials_affine_kernel<{rl}>": [("test_gpu_gn_fused.py", 'f"gn_partials_affine_kernel<{M.row_lanes(c, groups)}>"')] for rl in (4, 8)},
}

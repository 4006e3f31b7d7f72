"""The edge matrix of csrc/vmaf.hip, importable without a GPU: the case list, the inputs, the float64 expected values
(tests/_vmaf_ref.py, the statement of the contract), a restatement of the host's plan (passes, plane and band sizes,
tiles, the ADM window) from which the ledger (tests/test_vmaf_fvmd_ledger.py) derives what the cases reach, and the
mutants - the statement with one clause changed, each of which must move a named small case by at least 1e-6, a
thousand bars.

Every case is derived from a constant of the source: VMAF_PASS_FRAMES = 4 frames resident per pass, the 16 x 32 tile of
the VIF statistic and of motion, the 16 x 16 tile of the ADM pooling, the rounding step of `left = (int)(aw * 0.1 - 0.5)`,
the 4 waves of a predict workgroup and the 64 lanes over the support vectors, the 256 pixels of a luma workgroup.

The bar is the project's own, R.BAR = 1e-9 * max(1, |value|).  It holds only while every pixel falls the same way at the
one discontinuous branch, s1 >= nsq; `margin(case)` is the smallest |s1 - nsq| / nsq of a case and the ledger holds it to
1e-6 for every case.  An input that comes closer is to have its seed or amplitude changed, never the bar."""
import zlib
from dataclasses import dataclass
from functools import lru_cache
from typing import Optional

import numpy as np

import _vmaf_ref as R

BAR = R.BAR
PASS_FRAMES, TH, TW, AT, MIN_SIDE, THREADS, WAVE = 4, 16, 32, 16, 64, 256, 64      # the ledger reads them from the source
SOURCE = "vmaf.hip"
SIDES = (64, 65, 111, 120, 127, 129)
MARGIN = 1e-6

FEATURE_KERNELS = ("vmaf_vif_stat_kernel<17>", "vmaf_vif_stat_kernel<9>", "vmaf_vif_stat_kernel<5>", "vmaf_vif_stat_kernel<3>",
                   "vmaf_vif_down_kernel<9>", "vmaf_vif_down_kernel<5>", "vmaf_vif_down_kernel<3>", "vmaf_dwt_kernel<true>",
                   "vmaf_dwt_kernel<false>", "vmaf_adm_pool_kernel", "vmaf_motion_kernel", "vmaf_finish_kernel")


# ============================================================================================ cases
@dataclass(frozen=True)
class Case:
    id: str
    group: str                                # passes | neighbours | shapes | values
    h: int
    w: int
    n: int
    content: str = "fixture"                  # fixture | zero_full | full_full | checker | flat_ref | branch
    prev: bool = False
    following: bool = False

    @property
    def kernels(self):
        return FEATURE_KERNELS + (("vmaf_predict_kernel",) if self.group == "passes" else ())

    @property
    def seed(self):
        return zlib.crc32(self.id.encode())


def _build():
    cases = []
    for h, w, n in ((64, 64, 5), (64, 64, 8), (64, 64, 9), (66, 70, 6)):
        cases.append(Case(f"pass_{h}x{w}_n{n}", "passes", h, w, n))
    for n in (1, 5):
        for prev in (False, True):
            for following in (False, True):
                cases.append(Case(f"nb_n{n}_{'p' if prev else '-'}{'f' if following else '-'}", "neighbours", 64, 65, n, prev=prev,
                                  following=following))
    for h, w in ((64, 65), (65, 111), (111, 120), (120, 127), (127, 129), (129, 64), (120, 111), (129, 127), (65, 64), (127, 120)):
        cases.append(Case(f"shape_{h}x{w}", "shapes", h, w, 2))
    for content in ("zero_full", "full_full", "checker", "flat_ref"):
        cases.append(Case(f"value_{content}", "values", 64, 65, 2, content))
    cases.append(Case("value_branch_67x81", "values", 67, 81, 2, "branch"))
    assert len({c.id for c in cases}) == len(cases)
    return tuple(cases)


CASES = _build()
BY_ID = {c.id: c for c in CASES}


def of(group):
    return [c for c in CASES if c.group == group]


# entry point -> what elvis_last_launch reports after it; tests/test_gpu_vmaf_matrix.py asserts it after every call
NOTED = {"features": "vmaf_finish_kernel", "predict": "vmaf_predict_kernel", "luma": "vmaf_luma_kernel"}


def group_kernels():
    """group of tests/test_gpu_vmaf_matrix.py -> the kernels its cases launch."""
    out = {g: tuple(sorted({k for c in of(g) for k in c.kernels})) for g in ("passes", "neighbours", "shapes", "values")}
    out["predict"] = (NOTED["predict"],) if PREDICT_NSV and PREDICT_N and PREDICT_FLAGS else ()
    out["luma"] = (NOTED["luma"],) if LUMA else ()
    return out


# ============================================================================================ inputs
@lru_cache(maxsize=None)
def inputs(cid: str):
    """(ref, dis, prev or None, following or None): read-only u8 arrays, the same for every call."""
    c = BY_ID[cid]
    prev = nxt = None
    if c.content == "fixture":
        if c.group == "neighbours":               # the clip is frames 1 .. n of a fixture of n + 1; `prev` is frame 0, and
            r, d = R.fixture(c.h, c.w, c.n + 1)   # `following` the last frame's distorted twin: nearer than any frame of the
            ref, dis = r[1:], d[1:]               # clip is to its neighbour, so the minimum of motion2 takes it
            prev, nxt = (r[0] if c.prev else None), (d[c.n] if c.following else None)
        else:
            ref, dis = R.fixture(c.h, c.w, c.n)
    elif c.content == "zero_full":
        ref, dis = np.zeros((c.n, c.h, c.w), np.uint8), np.full((c.n, c.h, c.w), 255, np.uint8)
    elif c.content == "full_full":
        ref = dis = np.full((c.n, c.h, c.w), 255, np.uint8)
    elif c.content == "checker":                  # period 1, against its inverse; the second frame one pixel on
        yy, xx = np.mgrid[:c.h, :c.w]
        ref = np.stack([(((yy + xx + f) & 1) * 255).astype(np.uint8) for f in range(c.n)])
        dis = 255 - ref
    elif c.content == "flat_ref":                 # luma 128 is 0.0 after the offset: every reference coefficient is exactly 0
        ref = np.full((c.n, c.h, c.w), 128, np.uint8)
        dis = np.random.default_rng(c.seed).integers(0, 256, (c.n, c.h, c.w), dtype=np.uint8)
    elif c.content == "branch":
        ref, dis = R.branch_pair(c.h, c.w)
    else:
        raise ValueError(c.content)
    out = tuple(None if a is None else np.ascontiguousarray(a) for a in (ref, dis, prev, nxt))
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def expected(cid: str, mutant: Optional[str] = None):
    """The statement's features [n, 6] of a case, computed once and shared."""
    ref, dis, prev, nxt = inputs(cid)
    out = R.features(ref, dis, prev, nxt, mutant=mutant)
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def counts(cid: str):
    ref, dis, prev, nxt = inputs(cid)
    c = R.new_counts()
    R.features(ref, dis, prev, nxt, counts=c)
    return c


def margin(cid: str) -> float:
    """The smallest |s1 - nsq| / nsq over all scales, frames and pixels."""
    return min(counts(cid)["nsq_margin"])


# mutant -> the small case on which it must differ from `expected` by >= 1e-6
MUTANTS = {
    "mirror_repeats_edge": "shape_64x65",
    "decimate_odd": "shape_65x64",
    "adm_window_floor": "shape_120x111",
    "adm_threshold_no_centre": "shape_64x65",
    "motion2_before": "nb_n5_pf",
    "vif_tile_row_more": "shape_65x111",
    "pass2_from_0": "pass_64x64_n9",
    "adm_hw_swapped": "shape_127x129",
}
assert set(MUTANTS) == set(R.MUTANTS)


# ============================================================================================ the host's plan
def plan(h: int, w: int, n: int):
    """vmaf_plan and the pass loop of elvis_vmaf_features_f64, from the numbers alone: dict(passes = the frame count of
    each pass, vif = [(vh, vw)] and adm = [(ah, aw, top, left)] per scale)."""
    passes = [min(PASS_FRAMES, n - f0) for f0 in range(0, n, PASS_FRAMES)]
    vif, adm = [], []
    vh, vw, ah, aw = h, w, h, w
    for s in range(4):
        if s:
            vh, vw = vh // 2, vw // 2
        vif.append((vh, vw))
        ah, aw = (ah + 1) // 2, (aw + 1) // 2
        adm.append((ah, aw, max(0, int(ah * 0.1 - 0.5)), max(0, int(aw * 0.1 - 0.5))))
    return dict(passes=passes, vif=vif, adm=adm)


def case_plan(c: Case):
    return plan(c.h, c.w, c.n)


# ============================================================================================ predict and luma
PREDICT_NSV, PREDICT_N, PREDICT_FLAGS = (1, 63, 64, 65), (1, 4, 5), tuple(range(8))


def predict_model_fields(nsv: int, flags: int):
    """The fields of a VmafModel with `nsv` support vectors and the three flag bits: transform on (1), out >= in (2), the
    clip (4).  The clip is narrow and the transform bent enough for each to move some score of `predict_features`."""
    rng = np.random.default_rng(100 * nsv + flags)
    sv = rng.uniform(0.0, 1.0, (nsv, 6))
    coef = rng.uniform(0.5, 1.5, nsv) / nsv
    slopes = np.concatenate([[0.01], rng.uniform(0.8, 1.2, 6)])
    slopes[2] = 0.05
    intercepts = np.concatenate([[0.0], rng.uniform(-0.1, 0.1, 6)])
    return dict(slopes=slopes, intercepts=intercepts, sv=sv, coef=coef, rho=0.05, gamma=0.5,
                score_clip=(30.0, 50.0) if flags & 4 else None, transform=(40.0, -0.2, 0.004, bool(flags & 2)),
                enable_transform=bool(flags & 1))


def predict_features(n: int) -> np.ndarray:
    rng = np.random.default_rng(n)
    f = rng.uniform(0.0, 1.0, (n, 6))
    f[:, 1] = rng.uniform(0.0, 20.0, n)
    return f


def predict_waves(n: int):
    """(workgroups, waves of the last workgroup that have a frame)."""
    per = THREADS // WAVE
    return -(-n // per), (n - 1) % per + 1


# (frame shape n, h, w), then the rectangles (y0, y1, x0, x1) cut from it
LUMA = (((2, 20, 300), ((3, 4, 5, 6), (7, 8, 11, 268), (2, 17, 3, 20), (1, 17, 9, 25), (0, 20, 0, 300))),
        ((1, 260, 20), ((2, 259, 7, 8), (0, 1, 19, 20))))


def luma_inputs(shape):
    rng = np.random.default_rng(shape[1] * 1000 + shape[2])
    frames = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    masks = (rng.random(shape) < 0.6).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)
    return frames, masks


def luma_pixels():
    return sorted({(r[1] - r[0]) * (r[3] - r[2]) for _, rects in LUMA for r in rects})

"""The edge matrix of csrc/vmaf.hip on the device (tests/_vmafcases.py) against the numpy float64 statement of the
contract (tests/_vmaf_ref.py): clips of more than one pass of four frames, every combination of `prev` / `following`,
plane and band sizes on, one under and one over the tile sides and on both sides of the ADM window's rounding step, value
edges, every flag of the score over 1 / 63 / 64 / 65 support vectors, and the luma kernel's block edges.

Bound: the project's own, R.BAR = 1e-9 * max(1, |value|), as tests/test_gpu_vmaf.py carries it; nothing new.  It holds
because every case keeps |s1 - nsq| / nsq >= 1e-6 at the one discontinuous branch (tests/test_vmaf_fvmd_ledger.py)."""
import numpy as np
import pytest
import torch

import _vmaf_ref as R
import _vmafcases as K
from elvis_amd import _lib, vmaf

pytestmark = pytest.mark.gpu


def _dev(a, device):
    return None if a is None else torch.from_numpy(np.array(a)).to(device)          # a copy: the shared inputs are read-only


def _launch():
    return _lib.lib().elvis_last_launch().decode()


def _report(name, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    worst = float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()) if got.size else 0.0
    print(f"{name}: worst |device - statement| / max(1, |statement|) = {worst:.3g} (bar {R.BAR:g})")
    return worst


@pytest.fixture(scope="module")
def model():
    return vmaf.make_vmaf_model(0)


def _run(case, device):
    ref, dis, prev, nxt = (_dev(a, device) for a in K.inputs(case.id))
    feats = vmaf.vmaf_features_device(ref, dis, prev=prev, following=nxt)
    assert _launch() == K.NOTED["features"]
    assert feats.shape == (case.n, 6) and feats.dtype == torch.float64
    assert torch.equal(vmaf.vmaf_features_device(ref, dis, prev=prev, following=nxt), feats)        # two runs: the same bytes
    return ref, dis, feats


@pytest.mark.parametrize("case", K.of("passes"), ids=lambda c: c.id)
def test_more_than_one_pass(gpu_device, model, case):
    """n = 5, 8, 9 and 6: two and three passes, a last pass of 1, 2 and 4 frames.  A frame's features do not depend on how
    many frames a call is given: the clip in one call is the bytes of its frames one call each."""
    ref, dis, feats = _run(case, gpu_device)
    want = K.expected(case.id)
    for k, name in enumerate(R.FEATURES):
        _report(f"{case.id} {name}", feats[:, k].cpu().numpy(), want[:, k])
    assert _report(case.id, feats.cpu().numpy(), want) <= R.BAR
    single = [vmaf.vmaf_features_device(ref[f:f + 1], dis[f:f + 1], prev=ref[f - 1] if f else None,
                                        following=ref[f + 1] if f + 1 < case.n else None) for f in range(case.n)]
    assert torch.equal(torch.cat(single), feats)
    scores = vmaf.vmaf_device(ref, dis, model)
    assert _launch() == K.NOTED["predict"]
    want_scores = R.score(want, model)
    assert _report(f"{case.id} score", scores.cpu().numpy(), want_scores) <= R.BAR
    assert torch.equal(vmaf.vmaf_device(ref, dis, model), scores) and np.ptp(want_scores) > 0


@pytest.mark.parametrize("case", K.of("neighbours") + K.of("shapes") + K.of("values"), ids=lambda c: c.id)
def test_features_against_the_statement(gpu_device, case):
    _, _, feats = _run(case, gpu_device)
    want = K.expected(case.id)
    assert np.isfinite(want).all()
    assert _report(f"{case.group} {case.id}", feats.cpu().numpy(), want) <= R.BAR


@pytest.mark.parametrize("nsv", K.PREDICT_NSV)
def test_predict_flags_support_vectors_and_waves(gpu_device, nsv):
    """All 8 flag values; 1, 63, 64 and 65 support vectors over the 64 lanes; 1, 4 and 5 frames leave one wave, the four
    waves of a workgroup and a second workgroup with one."""
    worst = 0.0
    for flags in K.PREDICT_FLAGS:
        m = vmaf.VmafModel(**K.predict_model_fields(nsv, flags))
        assert m.flags == flags
        for n in K.PREDICT_N:
            feats = K.predict_features(n)
            got = vmaf.vmaf_predict_device(_dev(feats, gpu_device), m).cpu().numpy()
            assert _launch() == K.NOTED["predict"]
            want = R.score(feats, m)
            assert R.within_bar(got, want), (nsv, flags, n, got, want)
            worst = max(worst, float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()))
    print(f"predict nsv {nsv}: worst |device - statement| / max(1, |statement|) = {worst:.3g} (bar {R.BAR:g})")


@pytest.mark.parametrize("shape,rects", K.LUMA, ids=lambda v: "x".join(map(str, v)) if isinstance(v[0], int) else "")
def test_luma_block_edges(gpu_device, shape, rects):
    """Rectangles of 1, 255, 256 and 257 pixels (one workgroup less a lane, exactly one, one lane into a second), as one
    row and as one column, both orders, with and without masks, kept and inverted."""
    frames, masks = K.luma_inputs(shape)
    f_d, m_d = _dev(frames, gpu_device), _dev(masks, gpu_device)
    for rect in rects:
        for order in ("rgb", "bgr"):
            got = vmaf.luma_device(f_d, order, rect=rect).cpu().numpy()
            assert _launch() == K.NOTED["luma"]
            assert np.array_equal(got, R.luma(frames, order, rect=rect)), (rect, order)
            for invert in (False, True):
                got = vmaf.luma_device(f_d, order, masks=m_d, invert=invert, rect=rect).cpu().numpy()
                assert np.array_equal(got, R.luma(frames, order, masks, invert, rect)), (rect, order, invert)
    print(f"luma {shape}: {len(rects)} rectangles, both orders, plain / masked / inverted: the same bytes")

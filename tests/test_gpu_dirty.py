"""Every device surface returns the bytes its statement names whatever its fresh allocations held.

Each case of tests/_dirtycases.py runs with `torch.empty`, `torch.empty_like` and `Tensor.new_empty` poisoned
(tests/_dirty.py), once with every byte 0xFF and once with 0x7F.  Three things are checked:

  * the sites the ledger assigns to the case were really allocated from during the run;
  * the result equals the statement - byte for byte for the integer families, within the family's own bound (imported
    from its reference module or its GPU test, not restated) for the float ones;
  * the results under the two poisons are the same bytes, float families included: every atomic in csrc/ is an integer
    atomic, so the arithmetic is deterministic, and a float that absorbed one poison cannot have absorbed the other.

The inputs are uploaded inside the run too: an upload is a copy into a fresh allocation and must not care either.
"""
import numpy as np
import pytest
import torch

import _dirty
import _dirtycases as D

pytestmark = pytest.mark.gpu

_expected = {}           # case id -> the statement's value, computed once and left unchanged
_results = {}            # (case id, poison) -> ({name: ndarray | bytes}, sites seen); each pair runs once a session


def _host(v):
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().numpy()
    return v if isinstance(v, bytes) else np.asarray(v)


def _run(case, byte, device, monkeypatch):
    key = (case.id, byte)
    if key not in _results:
        if case.prepare is not None:
            case.prepare(device)
        with monkeypatch.context() as mp, torch.cuda.device(device):
            seen = _dirty.poison(mp, byte)
            probe = torch.empty(16, dtype=torch.uint8, device=device)
            assert bool((probe == byte).all()), "the poisoner is not in effect on the device"
            got = case.run(device)
            torch.cuda.synchronize(device)
            got = {name: _host(v) for name, v in got.items()}
        _results[key] = (got, frozenset(seen))
    return _results[key]


def _raw(v):
    return v if isinstance(v, bytes) else (str(v.dtype), v.shape, v.tobytes())


@pytest.mark.parametrize("byte", _dirty.POISONS, ids=lambda b: f"0x{b:02X}")
@pytest.mark.parametrize("cid", sorted(D.CASES))
def test_result_does_not_depend_on_fresh_allocations(gpu_device, monkeypatch, cid, byte):
    case = D.CASES[cid]
    got, seen = _run(case, byte, gpu_device, monkeypatch)
    print(f"{cid} 0x{byte:02X}: allocated from {sorted(s for s in seen if s[0].startswith('elvis_amd'))}")
    claimed = {site for site, entry in D.SITES.items() if entry[:2] == ("case", cid)}
    assert claimed <= seen, f"{cid}: the ledger says this case reaches {sorted(claimed - seen)}; the run allocated from {sorted(seen)}"
    if cid not in _expected:
        _expected[cid] = case.expected()
    case.compare(got, _expected[cid])
    other, _ = _run(case, next(b for b in _dirty.POISONS if b != byte), gpu_device, monkeypatch)
    assert set(other) == set(got)
    for name in got:
        assert _raw(got[name]) == _raw(other[name]), f"{cid}: {name} differs between the poisons 0xFF and 0x7F"

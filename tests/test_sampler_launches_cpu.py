"""The launches of the sgm sampler loops, entry by entry, against the recorded log of tests/golden/sampler_launches.json.

tests/test_sampler_loops_gpu.py bounds every loop per step against float64 on the device; this one needs no GPU and is exact: the
coefficient of every ln3d_lincomb / ln3d_edm_euler_step launch as the host float64 handed to ctypes, the order of the terms, which
buffer is `y` and which `out`, every network call's label and batch, every step_noise(i), and what the fused routes hand to
prepare_timesteps / mod_cache / in_scale (tests/sampler_launches.py has the format and regenerates the file).  A reassociated
coefficient, a reordered term or a moved network call is a different log."""
import json

import pytest

import sampler_launches as L
import sampler_refs as R

with open(L.GOLDEN) as _f:
    _GOLDEN = json.load(_f)['logs']


def test_golden_covers_every_case_and_shape():
    assert list(_GOLDEN) == [str(s) for s in R.SHAPES]
    for shape in _GOLDEN:
        assert list(_GOLDEN[shape]) == list(R.SGM_CASES)


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
@pytest.mark.parametrize("name", list(R.SGM_CASES))
def test_sgm_loop_launches_equal_the_recorded_log(name, shape):
    want, got = _GOLDEN[str(shape)][name], L.record(R.SGM_CASES[name], shape)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f'{name} {shape}: entry {i} of {len(want)} differs: got {g}, recorded {w}'
    longer = got if len(got) > len(want) else want
    assert len(got) == len(want), f'{name} {shape}: {len(got)} entries, recorded {len(want)}; first unmatched: {longer[min(len(got), len(want)):][:1]}'

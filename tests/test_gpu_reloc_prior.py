"""GPU tests of ptz_reloc_prior_pairs (csrc/ptz_reloc_prior.hip): the device is array-equal to the host instantiation of the shared
header (tests/cpu_harness/reloc_prior_harness.cc), which tests/test_cpu_reloc_prior.py holds to the numpy restatement -- at the edges
of the wave's stride over the references, for list lengths below and above the reference count, and whatever the batch."""
import os
import subprocess
import sys

import numpy as np
import pytest

import reloc_prior_harness as ph
import reloc_prior_util as pu

pytestmark = pytest.mark.gpu


def _case(n_ref, n_query, seed, **kw):
    cams = ph.make_cams(n_ref, seed, dist=True)
    pri, wh = ph.make_priors(n_query, seed + 50, dist=True, **kw)
    return cams, ph.rotations(cams), pri, ph.rotations(pri), wh


def _harness(c, ft, R, mo=8):
    cams, Rr, pri, Rq, wh = c
    return ph.harness_prior_pairs(cams, Rr, pri, Rq, wh, ft, R, mo)


def _device(pkg, c, ft, R, mo=8):
    cams, Rr, pri, Rq, wh = c
    return pkg.api.reloc_prior_pairs(cams, pri, wh, factor_type=ft, ref_R=Rr, prior_R=Rq, max_refs=R, min_overlap=mo)


@pytest.mark.parametrize("n_ref", [1, 2, 63, 64, 65, 130, 200])
def test_device_equals_harness_at_the_stride_edges(pkg, n_ref):
    """Five queries (one with the rig behind it, one looking away from every reference) for every list length and factor type."""
    c = _case(n_ref, 5, n_ref, behind=(1,), away=(3,))
    for R in (1, 4, 8, 70):
        for ft in ((0, 3) if R in (1, 70) else (1, 2)):
            got = _device(pkg, c, ft, R)
            pu.assert_equal(got, _harness(c, ft, R), (n_ref, R, ft))
            assert got["n_short"][1] == 0 and got["n_short"][3] == 0 and (got["overlap"][3] == 0).all() and (got["shortlist"][3] == -1).all()
    if n_ref >= 63:
        assert got["n_short"].max() > 8 and got["overlap"].max() > 64


@pytest.mark.parametrize("n_query", [0, 1, 5, 257])
def test_device_equals_harness_for_any_batch(pkg, n_query):
    c = _case(65, n_query, 7, behind=tuple(range(2, n_query, 9)), away=tuple(range(4, n_query, 11)))
    got = _device(pkg, c, 2, 8, mo=20)
    pu.assert_equal(got, _harness(c, 2, 8, mo=20), n_query)
    assert got["shortlist"].shape == (n_query, 8) and got["H_slot"].shape == (n_query, 8, 9)
    if n_query >= 5:
        assert got["n_short"][4] == 0 and got["n_short"].max() == 8


def test_a_query_returns_its_own_bits_alone_reversed_and_in_a_split_batch(pkg):
    c = _case(130, 9, 3, behind=(2,), away=(5,))
    cams, Rr, pri, Rq, wh = c
    whole = _device(pkg, c, 1, 8)
    sub = lambda qs: _device(pkg, (cams, Rr, pri[qs], Rq[qs], wh[qs]), 1, 8)
    rev = sub(np.arange(9)[::-1].copy())
    parts = [sub(np.arange(0, 4)), sub(np.arange(4, 9))]
    for k in pu.KEYS:
        assert np.array_equal(rev[k][::-1], whole[k]), k
        assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k]), k
        for q in (0, 2, 5, 8):
            assert np.array_equal(sub(np.array([q]))[k][0], whole[k][q]), (k, q)


def test_device_pointer_form_returns_the_host_forms_arrays():
    """ptz_reloc_prior_pairs_device on a stream, device inputs and outputs full of stale values: the host form's arrays.  Own process
    with torch initialised first (as test_gpu_desc_shortlist.py::test_device_form_and_stale_workspace)."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "run_reloc_prior_device.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and r.stdout.count("reloc prior device ok") == 3, r.stdout[-2000:] + r.stderr[-2000:]


def test_bad_arguments_are_refused_before_any_launch(pkg):
    c = _case(4, 3, 1)
    cams, Rr, pri, Rq, wh = c
    E = pkg.api.PtzError

    def code(**kw):
        a = dict(ref_cams=cams, prior_cams=pri, query_wh=wh, ref_R=Rr, prior_R=Rq)
        a.update(kw)
        with pytest.raises(E) as e:
            pkg.api.reloc_prior_pairs(**a)
        return e.value.code

    bad = pri.copy(); bad[1, 5] = np.nan
    assert code(prior_cams=bad) == -1
    bad = pri.copy(); bad[2, 12] = np.inf
    assert code(prior_cams=bad) == -1
    bad = pri.copy(); bad[0, 0] = 0.0
    assert code(prior_cams=bad) == -1
    assert code(max_refs=0) == -1 and code(min_overlap=129) == -1 and code(min_overlap=-1) == -1
    assert code(radius_px=0.0) == -1 and code(radius_px=float("nan")) == -1
    zero = wh.copy(); zero[1, 0] = 0
    assert code(query_wh=zero) == -1 and code(factor_type=4) == -4
    assert pkg.api.reloc_prior_pairs(cams, pri[:0], wh[:0])["shortlist"].shape == (0, 8)

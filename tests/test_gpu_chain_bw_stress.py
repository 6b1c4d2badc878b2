"""Stress of the Chain pullbacks against float64, elementwise: gnx_chain_block_backward (every Dense layer of the wide cases through dx_mfma under
bw_dx_chain and k_dw_gemm, with k_ln_backward<false>, bw_gelu_preact and bw_delta between them) and gnx_chain_block_backward_narrow
(k_chain_mlp_bw<WMAX, SRC>), on one batch of 131 graphs, 1031 nodes and 4099 edges — the graph level of the fused kernel runs two full waves, a
wave of 3 rows and a wave past the end; the node level 17 chunks, the last of 7 rows.  tests/chain_bw_cases.py holds the cases; three paths ran
nowhere in the suite before them: a LayerNorm in the sqrt-eps mode inside a Chain (N-ln-both-modes, N-log_uniform_inputs, N-gelu-hidden,
W-tails), an activation on a chain's last layer (N-last-act, N-last-act-gelu-edge, W-gelu-last-act) and a fused graph level of more than 64 rows
(every narrow case but N-R2, N-mixed and N-ln-sqrt-first).

One fresh child per form of the matrix-core products (tests/chain_bw_stress_child.py): the default form with GNX_FFN_FP32 / GNX_EDGE_FP32 removed
from its environment, then the fp32-instruction form with both set — one after the other, each under a timeout; when the first fails the second
is not started.  All comparing happens here, on the CPU, for each form, entry and tensor:
  a. everything is finite, and exactly 0 where S = 0;
  b. |got - ref| <= 1e-5 . S for every element of every gradient, S the first-order error scale of oracle/gn_oracle.py's
     chain_block_backward_sparse (tests/test_chain_bw_stress_cpu.py: never above the product rule's S, and plain torch float32 within a quarter
     of the bar on every case);
  c. tensors of >= 4096 elements: the mean of |got - ref| / S is at most 4 x that of plain torch float32 — this is the criterion that does not
     depend on how loose a worst-case S is behind three levels of sums, and the one that sees the CPU controls a and c;
  d. the set of tensor names, and the masks of both `_applies`; the old normwise bar 1e-3 . max(1, max|ref|) on every tensor as well (all but the
     cancelling sums, tests/chain_bw_cases.py: normwise_applies): where S is loose no tensor is held more loosely than before;
  e. the profiler's scopes (tests/chain_bw_cases.py: expected_scopes), and that the part-fused call (N-mixed) launches fewer kernels than the generic one;
  f. the forward outputs of both forward entries within 1e-5 . S of chain_block_forward_sparse;
  g. the cancelling cases cancel (median S / |ref| of the edge chain's first dW >= 1e4).
Each tensor prints one `CHAINBW` line — worst / bar, mean / yardstick and the normwise error over the old bar per form and entry —, recorded in profiles/chain_bw_stress.md, not asserted."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import bw_x6_cases as BC
from tests import chain_bw_cases as CC
from tests import util as U
from tests.test_gpu_bw_x6_stress import CHILD_TIMEOUT, FORM_VARS, FORMS, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gn():
    import graphnets_jl_amd as gn
    return gn


@pytest.fixture(scope="module")
def runs(gn, tmp_path_factory):
    """{form: the directory its child wrote, or a string saying how the child failed}; a form whose predecessor failed is absent"""
    U.needs_default_forms(gn, "FFN_FP32", "EDGE_FP32")
    out = {}
    for form in FORMS:
        env = {k: v for k, v in os.environ.items() if k not in FORM_VARS}
        if form == "fp32_instruction":
            env.update({k: "1" for k in FORM_VARS})
        d = tmp_path_factory.mktemp("chain_" + form)
        try:
            r = subprocess.run([sys.executable, "-m", "tests.chain_bw_stress_child", str(d)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            out[form] = f"child {form}: no result within {CHILD_TIMEOUT} s"
            break
        if r.returncode != 0:
            out[form] = f"child {form}: exit {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}"
            break
        out[form] = d
    return out


def _dir(runs, form):
    assert form in runs, f"the child of {form} was not started: {runs[FORMS[0]]}"
    assert not isinstance(runs[form], str), runs[form]
    return runs[form]


def _meta(runs, form):
    with open(os.path.join(_dir(runs, form), "meta.json")) as f:
        return json.load(f)


def _load(runs, form, cid, kind, entry):
    with np.load(os.path.join(_dir(runs, form), f"{cid}.{kind}.{entry}.npz")) as z:
        return {n: z[n] for n in z.files}


def test_each_form_ran_in_a_process_of_its_own(gn, runs):
    L = gn._lib
    for form, want in zip(FORMS, (0, L.FLAG_FFN_FP32 | L.FLAG_EDGE_FP32)):
        meta = _meta(runs, form)
        assert meta["flags"] & (L.FLAG_FFN_FP32 | L.FLAG_EDGE_FP32) == want, (form, hex(meta["flags"]))
        assert set(meta["scopes"]) == set(meta["masks"]) == set(CC.CASE_IDS)


@pytest.mark.parametrize("cid", CC.CASE_IDS)
def test_forward_within_1e5_S_of_float64(runs, cid):
    ref, S = CC.forward_reference(cid)
    failures = []
    for form in FORMS:
        for entry in CC.entries(cid):
            got = _load(runs, form, cid, "fw", entry)
            assert set(got) == {n for n in ref if ref[n] is not None}, (cid, form, entry, sorted(got))
            for n in sorted(got):
                (w, m), _ = BC.ratios(got[n], ref[n], S[n])
                print(f"CHAINFW {cid} {form} {entry} {n} size {ref[n].size}: worst/bar {w:.4f}")
                try:
                    BC.check_elementwise(got[n], ref[n], S[n], f"{cid} {form} {entry} {n}")
                except AssertionError as e:
                    failures.append(str(e))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("cid", CC.CASE_IDS)
def test_backward_within_1e5_S_of_float64_in_both_forms(runs, cid):
    ref, S, yard = CC.reference(cid)
    q = lambda a, b: a / b if b > 0 else (0.0 if a == 0 else float("inf"))
    figures, failures = {}, []
    for form in FORMS:
        meta = _meta(runs, form)
        assert meta["masks"][cid][1] == CC.want_mask(cid), (cid, form, meta["masks"][cid])
        if CC.CASE[cid]["family"] == "narrow":
            # the forward's rule takes whatever the backward's takes
            assert meta["masks"][cid][0] & meta["masks"][cid][1] == meta["masks"][cid][1], (cid, meta["masks"][cid])
        totals = {}
        for entry in CC.entries(cid):
            seen = meta["scopes"][cid][entry]
            must, must_not, kernels = CC.expected_scopes(cid, entry)
            assert must <= set(seen) and not (must_not & set(seen)) and not any(n.startswith("k_rows_gemm") for n in seen if entry == "narrow" and kernels), \
                f"{cid} {form} {entry}: missing {sorted(must - set(seen))}, unexpected {sorted(must_not & set(seen))}; saw {sorted(seen)}"
            for n, k in kernels.items():
                assert seen[n] == k, (cid, form, entry, n, seen[n])
            totals[entry] = sum(seen.values())
            got = _load(runs, form, cid, "bw", entry)
            assert set(got) == set(ref) == CC.grad_names(CC.data(cid)["p"]), (cid, form, entry, sorted(set(got) ^ set(ref)))
            for n in sorted(ref):
                (_, ym), _ = BC.ratios(yard[n], ref[n], S[n])
                (w, m), _ = BC.ratios(got[n], ref[n], S[n])
                figures[form, entry, n] = (w, q(m, ym), float(np.abs(got[n] - ref[n]).max()) / (CC.CHAIN_BAR * max(1.0, float(np.abs(ref[n]).max()))))
                try:
                    BC.check_elementwise(got[n], ref[n], S[n], f"{cid} {form} {entry} {n}")
                    BC.check_statistical(m, ym, ref[n].size, f"{cid} {form} {entry} {n}")
                    assert not CC.normwise_applies(cid, n) or BC.legacy_close(got[n], ref[n], CC.CHAIN_BAR), \
                        f"{cid} {form} {entry} {n}: max|got - ref| = {np.abs(got[n] - ref[n]).max():.3e} above 1e-3 . max(1, max|ref|)"
                except AssertionError as e:
                    failures.append(str(e))
        if cid == "N-mixed" and form == FORMS[0]:  # part fused: the fused node level replaces its generic launches by one kernel and its finishers
            assert totals["narrow"] < totals["generic"], (cid, form, totals)
    for n in sorted(ref):  # the record: printed before anything is asserted on the figures
        parts = [f"{form} {entry} worst/bar {figures[form, entry, n][0]:.4f} mean/yardstick {figures[form, entry, n][1]:.3f} normwise/old-bar {figures[form, entry, n][2]:.2e}" for form in FORMS for entry in CC.entries(cid)]
        print(f"CHAINBW {cid} {n} size {ref[n].size}: " + "; ".join(parts))
    assert not failures, "\n".join(failures)
    if CC.CASE[cid]["variant"] == "cancelling_dW":
        assert np.median(S["edge0.dW"] / (np.abs(ref["edge0.dW"]) + 1e-300)) >= 1e4

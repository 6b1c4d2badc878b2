"""Stress of the backward's matrix-core arithmetic against float64, elementwise.

tests/test_gpu_backward*.py hold the fp32 backward — the root of trust of all training code — to normwise bars (2e-4 / 1e-3 . max(1, max|ref|)) on
features in [0, 1): a backward that kept 16 mantissa bits would pass them 50 x over, and a wrong element that is small next to its tensor's largest
is invisible to them.  Here gnx_block_backward and gnx_core_backward run on inputs that stress the six-term products of k_dw_gemm (dW = X^T delta)
and k_rows_gemm (dX = delta W^T, with the act' epilogue and the column sums behind db1) — magnitudes over twelve decades in the features, the
cotangents and the weights, LayerNorm scales over six, sums that cancel to 1e-4 of their terms, widths with tails in every tile dimension — and every
element of every gradient is held to 1e-5 . S of the float64 pullback oracle (oracle/gn_oracle.py), S being the same pullback in absolute values.

The form of those products is read from the environment once per process and the backward's entry points take no flags, so one fresh child per
form (tests/bw_x6_stress_child.py) runs every case of tests/bw_x6_cases.py once: the default form with GNX_FFN_FP32 / GNX_EDGE_FP32 removed from its
environment, then the fp32-instruction form with both set — one after the other, each under a timeout; when the first fails the second is not
started.  All comparing happens here, on the CPU, for each form separately and for every gradient tensor:
  a. everything is finite, and exactly 0 where S = 0;
  b. |got - ref| <= 1e-5 . S for every element;
  c. tensors of >= 4096 elements: the mean of |got - ref| / S is at most 4 x that of the same pullback evaluated by plain torch float32 on the CPU
     (tests/test_bw_x6_stress_cpu.py: that evaluation keeps a 4 x margin to b on every case, a six-term product measures 0.5 - 0.9 x a torch fp32
     matmul and a product with 16 mantissa bits 14 - 26 x);
  d. the set of tensor names compared;
  e. the profiler's scope names: k_dw_gemm and the dX scopes wherever bw_use_mfma / bw_use_mfma_dw select them (C3 the dX scopes without
     k_dw_gemm), bw_gelu_preact for the gelu block, bw_gelu_hidden — the scope under which a core turns its recomputed hidden pre-activation into
     hidden units — for the gelu core.
Each tensor prints one `BWX6` line: its worst ratio to 1e-5 . S and its mean ratio to the yardstick per form, and the six-term / fp32-instruction
ratio of the means — recorded (profiles/bw_x6_stress.md), not asserted: the two forms sum in different orders."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import bw_x6_cases as BC
from tests import util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 600
FORM_VARS = ("GNX_FFN_FP32", "GNX_EDGE_FP32")
FORMS = ("six_terms", "fp32_instruction")


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
        d = tmp_path_factory.mktemp(form)
        try:
            r = subprocess.run([sys.executable, "-m", "tests.bw_x6_stress_child", str(d)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
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


def test_each_form_ran_in_a_process_of_its_own(gn, runs):
    L = gn._lib
    for form, want in zip(FORMS, (0, L.FLAG_FFN_FP32 | L.FLAG_EDGE_FP32)):
        with open(os.path.join(_dir(runs, form), "meta.json")) as f:
            meta = json.load(f)
        assert meta["flags"] & (L.FLAG_FFN_FP32 | L.FLAG_EDGE_FP32) == want, (form, hex(meta["flags"]))
        assert set(meta["scopes"]) == set(BC.CASE_IDS)


@pytest.mark.parametrize("cid", BC.CASE_IDS)
def test_backward_within_1e5_S_of_float64_in_both_forms(runs, cid):
    ref, S, yard = BC.reference(cid)
    must, must_not = BC.expected_scopes(cid)
    means, failures = {}, []
    for form in FORMS:
        d = _dir(runs, form)
        with open(os.path.join(d, "meta.json")) as f:
            seen = set(json.load(f)["scopes"][cid])
        assert must <= seen and not (must_not & seen), f"{cid} {form}: missing {sorted(must - seen)}, unexpected {sorted(must_not & seen)}; saw {sorted(seen)}"
        with np.load(os.path.join(d, cid + ".npz")) as z:
            got = {n: z[n] for n in z.files}
        assert set(got) == set(ref) == BC.names(cid), (cid, form, sorted(set(got) ^ set(ref)))
        for n in sorted(ref):
            (yw, ym), _ = BC.ratios(yard[n], ref[n], S[n])
            (w, m), _ = BC.ratios(got[n], ref[n], S[n])
            means[form, n] = (w, m, ym)
            try:
                BC.check_elementwise(got[n], ref[n], S[n], f"{cid} {form} {n}")
                BC.check_statistical(m, ym, ref[n].size, f"{cid} {form} {n}")
            except AssertionError as e:
                failures.append(str(e))
    for n in sorted(ref):  # the record: printed before anything is asserted on the figures
        (w6, m6, ym), (w32, m32, _) = means[FORMS[0], n], means[FORMS[1], n]
        q = lambda a, b: a / b if b > 0 else (0.0 if a == 0 else float("inf"))
        print(f"BWX6 {cid} {n} size {ref[n].size}: worst/bar six {w6:.4f} fp32 {w32:.4f}; mean/yardstick six {q(m6, ym):.3f} fp32 {q(m32, ym):.3f}; six/fp32 {q(m6, m32):.3f}")
    assert not failures, "\n".join(failures)
    if cid == "B1-cancelling_dW":
        assert np.median(S["grad.edgefn.dW"] / (np.abs(ref["grad.edgefn.dW"]) + 1e-300)) >= 1e4
    if cid == "B1-cancelling_dX":
        assert np.median(S["d_ef"] / (np.abs(ref["d_ef"]) + 1e-300)) >= 1e4

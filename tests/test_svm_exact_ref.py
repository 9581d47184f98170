"""CPU checks of the exact SVM reference (tests/svm_exact.py), of ero_svm_couple (the oracle's probability half on its own) and of the
str_er_svm_predict_probability_q8 surface (header, export, binding)."""
import ctypes as C
import gzip
import os
import re

import numpy as np
import pytest

import svm_exact as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# Both sides run the same f64 coupling (ero_svm_couple); on decision values a bound apart their probabilities differ by the sigmoid's slope times that
# bound, plus the rounding of an f64 fixed-point iteration of up to 100 sweeps over 65 classes: 100 x 65 x a few ulp of values below 1, under 1e-12.
# P_F64 allows a thousand times that.
P_F64 = 1e-9
# ... where the coupling does not stop near its threshold: the decision values' digit bounds (below 1e-7 on these models) move the stopping statistic
# by less than |probA| / 4 times that; MARGIN_F64 is ten times the largest such move
MARGIN_F64 = 1e-6


def _shipped(S, tmp_path, per_class):
    raw = gzip.open(S.cascade_io.ocr_model_path(per_class)).read()
    p = tmp_path / f"ocr{per_class}.model"
    p.write_bytes(raw)
    return str(p), E.Model(raw, 1800)


def _agree_with_oracle(m, osvm, q):
    """Decision values within the arithmetic bound plus what the model file's printed digits imply (the oracle evaluates the printed doubles,
    the reference the loader's bytes or f32 values); probabilities within the sigmoid's slope times that, where the coupling is not at its threshold."""
    K, dK = m.kernel(q)
    dec, _ = m.decision(K, dK)
    _, bound = m.decision(K, dK + E.digits_bound(m, q, K))
    lab, prob, sweeps, margin = E.couple(osvm, dec)
    for i in range(len(q)):
        ol, op, od = osvm.predict_probability(q[i] / 255.0)
        assert (np.abs(od - dec[i]) <= bound[i]).all(), (i, np.abs(od - dec[i]).max(), bound[i].max())
        if margin[i] > MARGIN_F64:
            assert np.abs(op - prob[i]).max() <= P_F64 + np.abs(m.probA).max() / 4 * bound[i].max() * E.SAFETY, i
    return dec


@pytest.mark.parametrize("per_class", [5, 120])
def test_reference_agrees_with_oracle_on_golden_vectors(S, oracle, tmp_path, per_class):
    from oracle.oracle import OracleSVM
    path, m = _shipped(S, tmp_path, per_class)
    assert m.form() == {"bytes": True, "class_sums": per_class == 120, "mode": 1, "msv": -1 if per_class == 120 else 5}
    z = np.load(os.path.join(GOLDEN, "svm_vectors120.npz" if per_class == 120 else "svm_vectors.npz"))
    osvm = OracleSVM(oracle, path)
    dec = _agree_with_oracle(m, osvm, z["q"])
    lab, prob, _, _ = E.couple(osvm, dec)
    assert (lab == z["label"]).all() and np.abs(prob - z["prob"]).max() < 1e-8


@pytest.mark.parametrize("byte", [True, False])
@pytest.mark.parametrize("k,lo,hi,empty,dim", [(2, 1, 5, (), 1), (7, 9, 14, (3,), 200), (66, 1, 6, (0,), 129)])
def test_reference_agrees_with_oracle_on_synthetic_models(oracle, tmp_path, k, lo, hi, empty, dim, byte):
    from oracle.oracle import OracleSVM
    rng = np.random.default_rng(31 * k + dim + byte)
    nsv = E.class_counts(rng, k, lo, hi, empty)
    text, svb = E.synth_model(rng, nsv, dim, byte)
    p = tmp_path / "m.model"
    p.write_bytes(text)
    m = E.Model(text, dim)
    assert m.bytes == byte and m.l == sum(nsv)
    _agree_with_oracle(m, OracleSVM(oracle, str(p)), E.near_vectors(rng, svb, 40))


def test_couple_reproduces_predict_probability(S, oracle, tmp_path):
    """ero_svm_couple on the oracle's own decision values is ero_svm_predict_probability's probability half, bit for bit."""
    from oracle.oracle import OracleSVM
    for per_class in (5, 120):
        path, _ = _shipped(S, tmp_path, per_class)
        osvm = OracleSVM(oracle, path)
        z = np.load(os.path.join(GOLDEN, "svm_vectors120.npz" if per_class == 120 else "svm_vectors.npz"))
        for x in z["q"][:16] / 255.0:
            lab, prob, dec = osvm.predict_probability(x)
            l2, p2, sweeps, margin = osvm.couple(dec)
            assert l2 == lab and np.array_equal(p2, prob) and 1 <= sweeps <= 100 and margin >= 0


def test_reference_form_follows_the_loader_rule():
    """svm_sv_bytes: a value more than 1e-3 / 255 off a numerator keeps the model out of the byte form; class sums from 9 support vectors a class."""
    base = "svm_type c_svc\nkernel_type rbf\ngamma 0.5\nnr_class 2\ntotal_sv {l}\nrho 0.1\nlabel 0 1\nprobA -1\nprobB 0\nnr_sv {a} {b}\nSV\n"
    for off, byte in ((0.0, True), (0.5e-3, True), (2e-3, False)):
        txt = base.format(l=2, a=1, b=1) + "1 0:%.17g\n-1 0:%.17g\n" % ((7 + off) / 255, 9 / 255)
        assert E.Model(txt, 1).bytes == byte
    txt = base.format(l=10, a=9, b=1) + "".join("1 0:%.17g\n" % (i / 255) for i in range(10))
    assert E.Model(txt, 1).form() == {"bytes": True, "class_sums": True, "mode": 0, "msv": -1}


def test_q8_entry_header_and_binding(S):
    txt = open(os.path.join(ROOT, "include", "str_er.h")).read()
    m = re.search(r"int\s+str_er_svm_predict_probability_q8\s*\(([^)]*)\)", txt)
    assert m, "str_er_svm_predict_probability_q8 not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert args == ["str_er_ctx *ctx", "const uint8_t *q", "int32_t n", "int32_t dim", "int32_t *label", "double *prob", "double *dec"], args
    L = S.load_library()
    assert hasattr(C.CDLL(S.lib_path()), "str_er_svm_predict_probability_q8")
    vp = C.c_void_p
    assert L.str_er_svm_predict_probability_q8.argtypes == [vp, vp, C.c_int32, C.c_int32, vp, vp, vp]
    assert callable(getattr(S.ERFilter, "svm_predict_q8"))

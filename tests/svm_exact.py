"""Exact reference of the OCR scorer's SVM half for vectors of 8-bit numerators over 255 (the vectors chain_run makes from its boxes), with an
error bound per decision value derived from the arithmetic of the device's forms.  Test infrastructure only (imported by tests/test_svm_exact*.py).

Which form the loader picks (api_models.cpp, svm_tables.h):
  bytes       every support-vector value is k / 255 to within 1e-3 / 255 (svm_sv_bytes): K from k_svm_kernel_i8, |x - sv|^2 an exact integer over 255^2
  bf16x3      any other model, vectors from boxes: k_svm_kernel_q, x.sv as three bf16 products per feature summed in f32
  f32         vectors handed in as doubles (str_er_svm_predict_probability): k_svm_kernel, f32(x).f32(sv) summed in f32
  class_sums  k <= 65 and more than 8 support vectors in some class: k_svm_decide's per-class f64 sums, then k_svm_couple<MODE, -1>
  MODE        k_svm_couple's build: 0 for k <= 64, 1 for k = 65, 2 for k >= 66;  MSV 5 (at most five a class), 0 (eights), -1 (class sums)

Reference.  K is computed from d2 in f64 (numpy exp, <= 1 ulp):
  bytes:  d2 = (sum a^2 + sum b^2 - 2 sum a b) / 65025 on the loader's bytes -- every sum is an integer below 2^53, so the f64 matrix product is exact
  others: d2 = |x|^2 + |sv|^2 - 2 x.sv in f64 on the f32 support vectors the device holds (x = q / 255); its own rounding is part of the bound below
Decision values are libsvm's pairing: dec(i, j) = av[i][j - 1] + av[j][i] - rho, av[c][s] = sum over class c's support vectors q of coef[s][q] K[q].

Bound.  u = 2^-53 (unit roundoff of f64), u32 = 2^-24 (of f32), gam(n) = n u / (1 - n u).
  d2 error, bytes: 0 (exact on both sides).
  d2 error, others: the device's f32 accumulation of x.sv over na roundings (na = dq for bf16x3: the three
    exact bf16 products of a feature count as one term, as in the design's estimate; dpad for f32) is at most gam32(na) S with S = sum |x_i sv_i|
    (the textbook bound of a recursive sum, any order); the f32 path also rounds x to f32 first: u32 S more;
    the f64 norms, the scaling by 2 / 255 and the final additions on both sides: gam(dim + 4) (|x|^2 + |sv|^2 + 2 S), twice (device and reference).
  K error: |dK| <= K expm1(gamma dd2) + (3 |arg| + 4) eps K, arg = -gamma d2, eps = 2^-52: the argument's three roundings (1 / 65025 or 2 / 255, the
    product with d2, the product with gamma) on each side are 3 |arg| eps; exp_neg (Cody-Waite reduction, degree-13 Taylor with truncation
    below 4.2e-18 relative, Horner in fused multiply-adds, ldexp) and numpy's exp (<= 1 ulp) are within 4 eps of exp together.
  decision value p = (i, j) over its n = nsv_i + nsv_j support vectors: sum |coef| |dK| + 2 gam(n + 1) (sum |coef K| + |rho|) -- the coefficient
    sums in f64 on both sides, in any order.
  The bound is multiplied by SAFETY (a named constant, at most 4) and nothing else.
Probabilities: ero_svm_couple (oracle/svm_oracle.c, the reference's sigmoid_predict + multiclass_probability) on the reference decision values.
"""
import gzip

import numpy as np

U64 = 2.0 ** -53
EPS64 = 2.0 ** -52
U32 = 2.0 ** -24
SAFETY = 2.0


def gam(n, u=U64):
    n = np.asarray(n, np.float64)
    return n * u / (1.0 - n * u)


def _align(v, a):
    return (v + a - 1) // a * a


class Model:
    """A libsvm text model (svm_save_model format, c_svc / rbf with probA / probB) as the device's loader sees it."""

    def __init__(self, text, dim):
        if isinstance(text, (bytes, bytearray)):
            text = text.decode()
        lines = text.split("\n")
        hdr, i = {}, 0
        while i < len(lines):
            ln = lines[i]
            i += 1
            key, _, rest = ln.partition(" ")
            if key == "SV":
                break
            hdr[key] = rest
        self.gamma = float(hdr["gamma"])
        self.k, self.l = int(hdr["nr_class"]), int(hdr["total_sv"])
        self.rho = np.array(hdr["rho"].split(), np.float64)
        self.probA = np.array(hdr["probA"].split(), np.float64)
        self.probB = np.array(hdr["probB"].split(), np.float64)
        self.label = np.array(hdr["label"].split(), np.int64)
        self.nsv = np.array(hdr["nr_sv"].split(), np.int64)
        self.start = np.concatenate([[0], np.cumsum(self.nsv)[:-1]]).astype(np.int64)
        k, l = self.k, self.l
        self.dim = dim
        self.coef = np.zeros((k - 1, l))
        self.sv = np.zeros((l, dim))                    # as parsed (strtod and float() both round correctly)
        for q in range(l):
            tok = lines[i + q].split()
            self.coef[:, q] = [float(t) for t in tok[:k - 1]]
            for t in tok[k - 1:]:
                a, b = t.split(":")
                self.sv[q, int(a)] = float(b)
        self.sv32 = self.sv.astype(np.float32).astype(np.float64)
        # the form (svm_sv_bytes, svm_uses_class_sums, launch_svm_couple)
        v = self.sv * 255.0
        qq = np.where(v < 0, -1.0, np.floor(v + 0.5))
        self.bytes = bool(((qq >= 0) & (qq <= 255) & (np.abs(v - qq) <= 1e-3)).all())
        self.sv8 = qq.astype(np.int64) if self.bytes else None
        self.msv = int(self.nsv.max())
        self.mp = 5 if self.msv == 5 else (self.msv + 7) // 8 * 8
        kc = _align(k - 1, 64)
        self.class_sums = k <= 65 and kc == 64 and self.mp > 8
        self.mode = 2 if k > 65 else (1 if k == 65 else 0)
        self.msv_build = -1 if self.class_sums else (5 if (k <= 65 and self.mp == 5) else 0)
        self.dq, self.dpad = _align(dim, 64), _align(dim, 16)

    @classmethod
    def from_path(cls, path, dim):
        raw = open(path, "rb").read()
        if raw[:2] == b"\x1f\x8b":
            raw = gzip.decompress(raw)
        return cls(raw, dim)

    def form(self):
        return {"bytes": self.bytes, "class_sums": self.class_sums, "mode": self.mode, "msv": self.msv_build}

    # ---- kernel values and their bound ----
    def kernel(self, q, path="q8"):
        """(K, dK bound) for vectors q [n x dim] of numerators, as scored by `path`: "q8" (the box path: bytes or bf16x3) or "f64" (vectors given as
        doubles q / 255: the f32 kernel)."""
        q = np.asarray(q)
        assert q.ndim == 2 and q.shape[1] == self.dim
        g = self.gamma
        if path == "q8" and self.bytes:
            a = q.astype(np.float64)
            b = self.sv8.astype(np.float64)
            ab = a @ b.T                                              # integers below 2^53: exact in any order
            d2i = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * ab
            assert (d2i >= 0).all()
            arg = -g * (d2i * (1.0 / 65025.0))
            dd2 = np.zeros_like(arg)
        else:
            x = q.astype(np.float64) / 255.0
            sv = self.sv32
            xn, sn = (x * x).sum(1)[:, None], (sv * sv).sum(1)[None, :]
            S = np.abs(x) @ np.abs(sv).T
            d2 = np.maximum(xn + sn - 2.0 * (x @ sv.T), 0.0)
            arg = -g * d2
            if path == "q8":
                acc = gam(self.dq, U32) * S
            else:
                acc = gam(self.dpad, U32) * S + U32 * S
            dd2 = 2.0 * acc + 2.0 * gam(self.dim + 4) * (xn + sn + 2.0 * S)
        K = np.exp(arg)
        dK = K * np.expm1(g * dd2) + (3.0 * np.abs(arg) + 4.0) * EPS64 * K
        return K, dK

    # ---- decision values and their bound ----
    def decision(self, K, dK):
        """(dec, bound) [n x k(k-1)/2] in libsvm's pair order."""
        k = self.k
        n = K.shape[0]
        ac = np.abs(self.coef)
        av = np.zeros((n, k, k - 1))                                 # av[c][s] = sum over class c of coef[s][q] K[q]
        ab = np.zeros((n, k, k - 1))                                 # the same of |coef| dK
        am = np.zeros((n, k, k - 1))                                 # the same of |coef K|
        for c in range(k):
            s0, s1 = self.start[c], self.start[c] + self.nsv[c]
            if s1 > s0:
                av[:, c] = K[:, s0:s1] @ self.coef[:, s0:s1].T
                ab[:, c] = dK[:, s0:s1] @ ac[:, s0:s1].T
                am[:, c] = K[:, s0:s1] @ ac[:, s0:s1].T
        ii, jj = np.triu_indices(k, 1)
        dec = av[:, ii, jj - 1] + av[:, jj, ii] - self.rho[None, :]
        nterm = (self.nsv[ii] + self.nsv[jj] + 1)[None, :]
        bound = ab[:, ii, jj - 1] + ab[:, jj, ii] + 2.0 * gam(nterm) * (am[:, ii, jj - 1] + am[:, jj, ii] + np.abs(self.rho)[None, :])
        return dec, SAFETY * bound

    def max_kernel(self, K):
        return K.max(axis=1) if K.shape[1] else np.zeros(K.shape[0])


def couple(osvm, dec):
    """Reference probabilities: ero_svm_couple per vector -> (label, prob, sweeps, margin)."""
    n = dec.shape[0]
    lab = np.zeros(n, np.int64)
    prob = np.zeros((n, osvm.k))
    sweeps = np.zeros(n, np.int64)
    margin = np.zeros(n)
    for i in range(n):
        lab[i], prob[i], sweeps[i], margin[i] = osvm.couple(dec[i])
    return lab, prob, sweeps, margin


def digits_bound(m, q, K):
    """How far the oracle (which evaluates sum (x - sv)^2 on the model's doubles as printed) may be from the reference above (the loader's bytes or
    f32 values): per kernel value, from d = |sv_printed - sv_used| elementwise, |dd2| <= 2 sum (|x| + |sv|) d + sum d^2 plus the oracle's own f64 sum of
    dim squares -> |dK| <= K expm1(gamma dd2)."""
    x = np.asarray(q, np.float64) / 255.0
    used = m.sv8 / 255.0 if m.bytes else m.sv32
    d = np.abs(m.sv - used)
    dd2 = 2.0 * (np.abs(x) @ d.T + (np.abs(m.sv) * d).sum(1)[None, :]) + (d * d).sum(1)[None, :]
    d2 = -np.log(np.maximum(K, 1e-300)) / m.gamma
    dd2 = dd2 + gam(m.dim + 2) * 2.0 * d2
    return K * np.expm1(m.gamma * dd2)


# ---- synthetic models and vectors near their support vectors ----
def class_counts(rng, k, lo, hi, empty=(), l_mod=None, top=None):
    """Support vectors per class: uniform in [lo, hi], classes `empty` without any, `top` (if given) forced on one class, the total adjusted
    to l_mod modulo 64."""
    nsv = rng.integers(lo, hi + 1, k)
    live = [c for c in range(k) if c not in empty]
    if top is not None:
        nsv[live[len(live) // 2]] = top
    for c in empty:
        nsv[c] = 0
    adj = [c for c in live if top is None or c != live[len(live) // 2]]
    if l_mod is not None:
        fixed = int(nsv.sum()) - int(nsv[adj].sum())
        lo_t, hi_t = fixed + lo * len(adj), fixed + hi * len(adj)
        s = int(nsv.sum())
        cands = [t for t in range(lo_t, hi_t + 1) if t % 64 == l_mod]
        assert cands, (k, lo, hi, l_mod)
        t = min(cands, key=lambda v: abs(v - s))
        while s != t:                                       # one step toward the target on a class that can take it
            c = adj[int(rng.integers(len(adj)))]
            if s < t and nsv[c] < hi:
                nsv[c] += 1; s += 1
            elif s > t and nsv[c] > lo:
                nsv[c] -= 1; s -= 1
    return [int(v) for v in nsv]


def synth_model(rng, nsv, dim, byte=True):
    """A libsvm text model whose support vectors lie near one random byte vector (so that kernel values between them are substantial): each is that
    vector with max(1, dim / 20) bytes moved by up to 30.  byte: values written as exact k / 255 doubles (%.17g), the loader's byte form; otherwise each
    numerator is off an integer by 0.1 .. 0.4, the bf16x3 form.  Returns (text, the support vectors' numerators rounded to bytes [l x dim])."""
    k, l = len(nsv), int(sum(nsv))
    mv = max(1, dim // 20)
    base = rng.integers(0, 256, dim)
    svb = np.repeat(base[None], l, 0)
    for q in range(l):
        pos = rng.choice(dim, size=mv, replace=False)
        svb[q, pos] = np.clip(svb[q, pos] + rng.integers(-30, 31, mv), 0, 255)
    num = svb.astype(np.float64) + (0.0 if byte else rng.uniform(0.1, 0.4, svb.shape))
    gamma = 0.7 / (mv * 0.0095)
    npairs = k * (k - 1) // 2
    f = lambda v: "%.17g" % v
    out = ["svm_type c_svc", "kernel_type rbf", "gamma " + f(gamma), f"nr_class {k}", f"total_sv {l}",
           "rho " + " ".join(f(v) for v in rng.normal(0, 0.5, npairs)), "label " + " ".join(str(i) for i in range(k)),
           "probA " + " ".join(f(v) for v in rng.uniform(-3, -0.5, npairs)), "probB " + " ".join(f(v) for v in rng.normal(0, 0.3, npairs)),
           "nr_sv " + " ".join(str(v) for v in nsv), "SV"]
    for q in range(l):
        co = " ".join(f(v) for v in rng.normal(0, 1.0, k - 1))
        feats = " ".join(f"{j}:{f(num[q, j] / 255.0)}" for j in range(dim) if num[q, j] != 0)
        out.append(co + " " + feats + " ")
    return ("\n".join(out) + "\n").encode(), np.clip(np.floor(num + 0.5), 0, 255).astype(np.uint8)


def near_vectors(rng, svb, n):
    """n vectors of numerators: exact copies of support vectors, copies with a few bytes moved, all 0, all 255 and random ones."""
    l, dim = svb.shape
    kind = rng.choice(5, size=n, p=[0.3, 0.5, 0.05, 0.05, 0.1])
    kind[: min(n, 5)] = np.arange(min(n, 5))            # (every kind at least once where n allows)
    q = np.zeros((n, dim), np.uint8)
    for i in range(n):
        if kind[i] <= 1:
            q[i] = svb[int(rng.integers(l))]
            if kind[i] == 1:
                mv = max(1, dim // 50)
                pos = rng.choice(dim, size=mv, replace=False)
                q[i, pos] = np.clip(q[i, pos].astype(np.int64) + rng.integers(-10, 11, mv), 0, 255)
        elif kind[i] == 2:
            q[i] = 0
        elif kind[i] == 3:
            q[i] = 255
        else:
            q[i] = rng.integers(0, 256, dim)
    return q

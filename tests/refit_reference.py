"""The float64 rule of the refit frontier (include/freud_sae.h, sae_refit_files) and the bounds its tests hold the engine to.

The rule.  Per frame: r_0 (the fp32 residual float(x) - b, taken as exact input), the operand rows w_s of its K slots (bf16 values),
the active flags.  Slots are visited in order; an active slot's PIVOT RATIO is |w_s - P w_s|^2 / |w_s|^2, P the projector on the
slots kept so far (float64, Gram-Schmidt with re-orthogonalisation); it is kept iff the ratio exceeds 2^-10.  e_s is the squared
error of the least-squares fit of r_0 on the kept slots among the first s: |r_0 - Q Q^T r_0|^2 with Q the orthonormal basis -- the
same number numpy.linalg.lstsq returns on every prefix (tests/test_refit_cpu.py holds the two against each other).  A slot is
DECIDED when its ratio lies outside [2^-11, 2^-9]; a frame is compared only if all its slots are decided.

The bounds, with U = 2^-24, gamma(n) = n U / (1 - n U), C = d_p / 64 columns per lane, for a frame with e_0 = |r_0|^2:

* Gram:  |G - G64| <= gamma(d_p) sum_e |w_s[e] w_t[e]|  (the header's bound: d_p exact products, at most d_p roundings in any order).
* c:     |c - c64| <= gamma(C + 32) sum_e |r_0[e] w_s[e]|  (a lane's chain of C fmaf, 31 additions per half, one to join them).
* e_0:   |e_0 - e_0,64| <= gamma(C + 32) e_0.
* the curve.  Backward errors first.  The factorisation computes the exact factor of G + dG with |dG_st| <= gamma(K + 1) (|L| |L|^T)_st
  (Higham, Accuracy and Stability, thm 10.3; the division by d_t and the correctly rounded root are inside K + 1), and
  (|L| |L|^T)_st <= sqrt(G_ss G_tt) = |w_s| |w_t| because row s of L has squared norm G_ss.  The forward substitution adds another
  gamma(K + 1) |L| on the factor.  With the Gram bound, the computed y is the exact one of a system perturbed by
      |dG_st| <= eps_G |w_s| |w_t|,  eps_G = gamma(d_p) + 2 gamma(K + 2);      |dc_s| <= eps_c sqrt(e_0) |w_s|,  eps_c = gamma(C + 32).
  The prefix error is f(G, c) = e_0 - c^T G^-1 c, so to first order df = a^T dG a - 2 a^T dc with a = G^-1 c the float64 coefficients:
      |df| <= eps_G S^2 + 2 eps_c sqrt(e_0) S,   S = sum_i |a_i| |w_i|.
  S is bounded through the NORMALISED Gram matrix of the frame's kept slots, lambda = its smallest eigenvalue (every prefix has a
  smallest eigenvalue at least as large, by interlacing): the normalised coefficients D a solve W^ (D a) = P r_0, so
  |D a|_2 <= sqrt(e_0 / lambda) and S = |D a|_1 <= sqrt(s e_0 / lambda).  Hence, with a factor 2 for the second-order terms (valid
  while eps_G K / lambda <= 0.1, asserted) and the chain e_{s+1} = fl(e_s - y_s^2) (one rounding of a number <= e_0 per step) on
  top of e_0's own error:
      |e_s - e_s64| <= [ 2 (eps_G s / lambda + 2 eps_c sqrt(s / lambda)) + (s + C + 32) U ] e_0.
  lambda <= the smallest kept pivot ratio, so this is the "K U e_0 / smallest ratio" scaling with the worst-case constants
  spelled out; at d_p = 256, K = 64 and lambda = 0.25 it is 1.3e-2 e_0, five decades above what random data shows (2.3e-7 e_0) --
  gamma(d_p) is a worst case and the tests' inputs are not.  curve_bound() returns it per frame and s.
* e_final.  The walk r = fmaf(-a_s, w, r) makes at most K roundings per element on magnitudes <= |r_0| + sum |a_i| |w_i|, so
  |dr|_2 <= gamma(K) (1 + sqrt(K / lambda)) sqrt(e_0) =: rho sqrt(e_0); the computed a differs from the float64 one by da with
  |W da|_2 <= sqrt(K / lambda) (eps_c + eps_G sqrt(K / lambda)) sqrt(e_0) =: eta sqrt(e_0), and the exact residual of the computed
  a is e_K64 + |W da|^2 (the least-squares residual is orthogonal to W).  The norm adds gamma(C + 32).  So
      |e_final - e_K64| <= [ 2 eta^2 + 2 (1 + eta) rho + rho^2 + gamma(C + 32) (1 + eta + rho)^2 ] e_0,
  and |e_final - e_K| is that plus the curve bound at K.  final_bound() returns the sum."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
DEP = 2.0 ** -10
DECIDED_LO, DECIDED_HI = 2.0 ** -11, 2.0 ** -9


def gamma(n):
    return n * U / (1 - n * U)


def round_up(a, b):
    return (a + b - 1) // b * b


def bf16(a):
    """float32 array rounded to the nearest bf16 value (ties to even), as float32."""
    a = np.ascontiguousarray(a, np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).reshape(a.shape)


class Frame:
    """The float64 rule on one frame: e [K + 1], ratio [K] (nan on a slot that is not active), kept [K], lam (the smallest
    eigenvalue of the normalised Gram matrix of the kept slots; 1 without any), coef [K] (the least-squares coefficients at K)."""

    def __init__(self, w, active, r0):
        w = np.asarray(w, np.float64)
        r0 = np.asarray(r0, np.float64)
        K, d = w.shape
        Q = np.zeros((d, K))
        nk = 0
        self.e0 = float(r0 @ r0)
        e = [self.e0]
        self.ratio = np.full(K, np.nan)
        self.kept = np.zeros(K, bool)
        for s in range(K):
            if active[s]:
                v = w[s]
                g = float(v @ v)
                q = v.copy()
                for _ in range(2):
                    q -= Q[:, :nk] @ (Q[:, :nk].T @ q)
                self.ratio[s] = float(q @ q) / g if g > 0 else 0.0
                if self.ratio[s] > DEP:
                    Q[:, nk] = q / np.sqrt(q @ q)
                    nk += 1
                    self.kept[s] = True
            res = r0 - Q[:, :nk] @ (Q[:, :nk].T @ r0)
            e.append(float(res @ res))
        self.e = np.array(e)
        self.K, self.d = K, d
        wk = w[self.kept]
        if nk:
            wn = wk / np.linalg.norm(wk, axis=1, keepdims=True)
            self.lam = float(np.linalg.eigvalsh(wn @ wn.T)[0])
            self.coef = np.zeros(K)
            self.coef[self.kept] = np.linalg.lstsq(wk.T, r0, rcond=None)[0]
        else:
            self.lam = 1.0
            self.coef = np.zeros(K)

    @property
    def decided(self):
        r = self.ratio[~np.isnan(self.ratio)]
        return bool(((r < DECIDED_LO) | (r > DECIDED_HI)).all())

    def eps(self, d_p):
        C = d_p // 64
        return gamma(d_p) + 2 * gamma(self.K + 2), gamma(C + 32)

    def curve_bound(self, d_p):
        """float64 [K + 1]: the bound on |e_s - e_s64|."""
        eg, ec = self.eps(d_p)
        assert eg * self.K / self.lam <= 0.1, f"the first-order bound needs eps_G K / lambda <= 0.1 (lambda = {self.lam:.3e})"
        s = np.arange(self.K + 1, dtype=np.float64)
        return (2 * (eg * s / self.lam + 2 * ec * np.sqrt(s / self.lam)) + (s + d_p // 64 + 32) * U) * self.e0

    def final_bound(self, d_p):
        """The bound on |e_final - e_K| (the fp32 curve's last entry)."""
        eg, ec = self.eps(d_p)
        K, g = self.K, gamma(d_p // 64 + 32)
        kl = np.sqrt(K / self.lam)
        eta = kl * (ec + eg * kl)
        rho = gamma(K) * (1 + kl)
        return (2 * eta ** 2 + 2 * (1 + eta) * rho + rho ** 2 + g * (1 + eta + rho) ** 2) * self.e0 + self.curve_bound(d_p)[K]


def lstsq_prefix_errors(w, kept, r0):
    """The rule as numpy.linalg.lstsq states it: the squared error of the least-squares fit on the kept slots of every prefix."""
    w = np.asarray(w, np.float64)
    r0 = np.asarray(r0, np.float64)
    out = [float(r0 @ r0)]
    for s in range(1, w.shape[0] + 1):
        wk = w[:s][kept[:s]]
        if wk.shape[0] == 0:
            out.append(out[0])
            continue
        a = np.linalg.lstsq(wk.T, r0, rcond=None)[0]
        res = r0 - wk.T @ a
        out.append(float(res @ res))
    return np.array(out)


def gram_bound(w, d_p):
    """float64 [K, K]: gamma(d_p) sum_e |w_s[e] w_t[e]|."""
    a = np.abs(np.asarray(w, np.float64))
    return gamma(d_p) * (a @ a.T)


def c_bound(w, r0, d_p):
    return gamma(d_p // 64 + 32) * (np.abs(np.asarray(w, np.float64)) @ np.abs(np.asarray(r0, np.float64)))


def r0_fp32(x, b):
    """float32 r_0 = float(x) - b, one fp32 subtraction."""
    x = np.asarray(x, np.float32)
    return x if b is None else (x - np.asarray(b, np.float32)).astype(np.float32)


def frames(w_rows, active, r0):
    """Frame objects for a batch: w_rows [R, K, d], active [R, K], r0 [R, d]."""
    return [Frame(w_rows[r], active[r], r0[r]) for r in range(len(r0))]


def assert_decided(fs, ctx=""):
    """At most 1 % of the frames may be undecided -> the mask of the decided ones."""
    dec = np.array([f.decided for f in fs])
    assert (~dec).sum() <= 0.01 * len(fs), f"{ctx}: {(~dec).sum()} of {len(fs)} frames undecided"
    return dec


# ---- the host half of freud_amd/csrc/refit_chol.h (and frontier.h) as a stand-alone program: the serial rule the kernel must
# reproduce to the bit.  Input: int32 mode, rows, K, d_p, has_b, 0; then per mode
#   0 (frame)   b [d_p] if has_b; per row: active u8 [K], w f32 [K][d_p], x f32 [d_p]  -> G [(K + 1) K], y, d, e [K + 1], a, e_final,
#               kept (as float), dep u8 [K]
#   1 (replay)  per row: active u8 [K], G f32 [(K + 1) K] (row K: c), e0 f32          -> y, d, e [K + 1], a, kept (as float), dep u8 [K]
#   2 (bins)    rows floats                                                          -> int32 bins
#   3 (e0)      b [d_p] if has_b; per row x f32 [d_p]                                -> e_0 by fr_row_serial
SERIAL_SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "refit_chol.h"
template <class V> static bool rd(FILE* f, V& v) { return v.empty() || fread(v.data(), sizeof(v[0]), v.size(), f) == v.size(); }
template <class V> static void wr(const V& v) { fwrite(v.data(), sizeof(v[0]), v.size(), stdout); }
int main(int argc, char** argv) {
  FILE* fp = argc > 1 ? fopen(argv[1], "rb") : NULL;
  int32_t h[6];
  if (!fp || fread(h, 4, 6, fp) != 6) return 2;
  const int mode = h[0], rows = h[1], K = h[2], d_p = h[3], has_b = h[4];
  if (mode == 2) {
    std::vector<float> v(rows);
    if (!rd(fp, v)) return 2;
    std::vector<int32_t> o(rows);
    for (int r = 0; r < rows; ++r) o[r] = rf_ratio_bin(v[r]);
    wr(o);
    return 0;
  }
  if (K < 0 || K > RF_MAX_K || d_p % 128 || d_p > FR_MAX_D) return 2;
  std::vector<float> b(has_b ? d_p : 0), x(d_p), w((size_t)K * d_p), G((size_t)(K + 1) * K), L((size_t)K * K), y(K), d(K), e(K + 1), a(K), one(1);
  std::vector<uint8_t> act(K), dep(K);
  if (!rd(fp, b)) return 2;
  for (int r = 0; r < rows; ++r) {
    if (mode == 0) {
      if (!rd(fp, act) || !rd(fp, w) || !rd(fp, x)) return 2;
      float ef;
      const int kept = rf_frame_serial(K, w.data(), act.data(), x.data(), has_b ? b.data() : NULL, d_p, G.data(), L.data(), y.data(), d.data(),
                                       e.data(), dep.data(), a.data(), &ef);
      wr(G); wr(y); wr(d); wr(e); wr(a);
      one[0] = ef; wr(one);
      one[0] = (float)kept; wr(one);
      wr(dep);
    } else if (mode == 1) {
      if (!rd(fp, act) || !rd(fp, G) || !rd(fp, one)) return 2;
      const int kept = rf_row_serial(K, G.data(), K, G.data() + (size_t)K * K, one[0], act.data(), L.data(), y.data(), d.data(), e.data(),
                                     dep.data(), a.data());
      wr(y); wr(d); wr(e); wr(a);
      one[0] = (float)kept; wr(one);
      wr(dep);
    } else {
      if (!rd(fp, x)) return 2;
      int bud;
      fr_row_serial(0, NULL, NULL, x.data(), has_b ? b.data() : NULL, d_p, NULL, 0, e.data(), &bud);
      one[0] = e[0]; wr(one);
    }
  }
  return 0;
}
"""


def build_serial(tmpdir, root):
    """Compile SERIAL_SRC (g++ -Wall -Werror -ffp-contract=off) -> the program's path."""
    import os
    import subprocess
    src, exe = os.path.join(str(tmpdir), "rf.cpp"), os.path.join(str(tmpdir), "rf")
    with open(src, "w") as f:
        f.write(SERIAL_SRC)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", f"-I{root}/freud_amd/csrc", src, "-o", exe], check=True)
    return exe


def _run(prog, tmpdir, blob):
    import os
    import subprocess
    path = os.path.join(str(tmpdir), "in.bin")
    with open(path, "wb") as f:
        f.write(b"".join(blob))
    return subprocess.run([prog, path], check=True, capture_output=True).stdout


def pad(a, d_p):
    a = np.asarray(a, np.float32)
    out = np.zeros(a.shape[:-1] + (d_p,), np.float32)
    out[..., :a.shape[-1]] = a
    return out


def _split(raw, rows, fields):
    """raw bytes -> dict of arrays: fields is a list of (name, count, dtype) per row."""
    dt = np.dtype([(n, t, (c,)) for n, c, t in fields])
    rec = np.frombuffer(raw, dtype=dt, count=rows)
    return {n: rec[n].copy() for n, _, _ in fields}


def serial_frames(prog, tmpdir, w_rows, active, x, b):
    """rf_frame_serial on rows: w_rows [R, K, d], active [R, K], x [R, d], b [d] or None -> dict (G [R, K + 1, K], y, d, e, a, e_final,
    kept, dep)."""
    R, K, dd = w_rows.shape
    d_p = round_up(dd, 128)
    blob = [np.array([0, R, K, d_p, int(b is not None), 0], np.int32).tobytes()]
    if b is not None:
        blob.append(pad(b, d_p).tobytes())
    wp, xp = pad(w_rows, d_p), pad(x, d_p)
    for r in range(R):
        blob += [np.asarray(active[r], np.uint8).tobytes(), wp[r].tobytes(), xp[r].tobytes()]
    o = _split(_run(prog, tmpdir, blob), R, [("G", (K + 1) * K, "<f4"), ("y", K, "<f4"), ("d", K, "<f4"), ("e", K + 1, "<f4"), ("a", K, "<f4"),
                                             ("e_final", 1, "<f4"), ("kept", 1, "<f4"), ("dep", K, "u1")])
    o["G"] = o["G"].reshape(R, K + 1, K)
    return o


def serial_replay(prog, tmpdir, gram, e0, active):
    """rf_row_serial on the engine's own trace: gram [R, K + 1, K], e0 [R], active [R, K] -> dict (y, d, e, a, kept, dep)."""
    R, K = active.shape
    blob = [np.array([1, R, K, 128, 0, 0], np.int32).tobytes()]
    g = np.ascontiguousarray(gram, np.float32)
    for r in range(R):
        blob += [np.asarray(active[r], np.uint8).tobytes(), g[r].tobytes(), np.float32(e0[r]).tobytes()]
    return _split(_run(prog, tmpdir, blob), R, [("y", K, "<f4"), ("d", K, "<f4"), ("e", K + 1, "<f4"), ("a", K, "<f4"), ("kept", 1, "<f4"),
                                               ("dep", K, "u1")])


def serial_bins(prog, tmpdir, values):
    v = np.ascontiguousarray(values, np.float32)
    return np.frombuffer(_run(prog, tmpdir, [np.array([2, v.size, 0, 128, 0, 0], np.int32).tobytes(), v.tobytes()]), np.int32).copy()


def serial_e0(prog, tmpdir, x, b):
    """e_0 of every row by the frontier's fr_row_serial."""
    R, dd = x.shape
    d_p = round_up(dd, 128)
    blob = [np.array([3, R, 0, d_p, int(b is not None), 0], np.int32).tobytes()]
    if b is not None:
        blob.append(pad(b, d_p).tobytes())
    blob.append(pad(x, d_p).tobytes())
    return np.frombuffer(_run(prog, tmpdir, blob), np.float32).copy()

"""Writes tests/golden/boys_seams.npz: the Boys function F_m(T) = int_0^1 t^(2m) exp(-T t^2) dt, m = 0 .. 20, with mpmath at 50 digits,
at the arguments where the implementations change branch (tests/eri_shapes.py: the Taylor grid of step 1/8 below T = 36 whose index
rounds up at 0.0625, 0.1875, 17.9375 and 35.9375, the asymptotic branch from 36 on; the oracle's own seams at 45, 50 and 65):
0, 1e-300, 1e-16, 1e-8; each seam with both neighbouring doubles and with a relative step of 2^-40 to either side; 100, 1e4, 1e7.
Run where mpmath is installed; no test imports it:    python tools/make_golden_boys_seams.py"""
import os

import mpmath as mp
import numpy as np

M_MAX = 20
SEAMS = (0.0625, 0.1875, 17.9375, 35.9375, 36.0, 45.0, 50.0, 65.0)


def arguments():
    out = [0.0, 1e-300, 1e-16, 1e-8]
    for s in SEAMS:
        out += [s * (1.0 - 2.0 ** -40), float(np.nextafter(s, -np.inf)), s, float(np.nextafter(s, np.inf)), s * (1.0 + 2.0 ** -40)]
    return out + [100.0, 1e4, 1e7]


def boys(m, T):
    """F_m(T) of the double T, by two routes that must agree: 1F1(m + 1/2; m + 3/2; -T) / (2m + 1), and for T > 0 the lower incomplete
    gamma function gamma(m + 1/2, T) / (2 T^(m + 1/2))"""
    T = mp.mpf(T)
    a = mp.mpf(m) + mp.mpf(1) / 2
    f1 = mp.hyp1f1(a, a + 1, -T) / (2 * m + 1)
    if T > 0:
        f2 = mp.gammainc(a, 0, T) / (2 * mp.power(T, a))
        assert abs(f1 - f2) <= mp.mpf(10) ** -40 * abs(f1), (m, T, f1, f2)
    return f1


def main():
    mp.mp.dps = 50
    T = np.asarray(arguments(), dtype=np.float64)
    F = np.asarray([[float(boys(m, t)) for m in range(M_MAX + 1)] for t in T])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "boys_seams.npz")
    np.savez(path, T=T, F=F)
    print(f"{os.path.normpath(path)}: {len(T)} arguments x {M_MAX + 1} orders")


if __name__ == "__main__":
    main()

"""Derive the polynomial coefficients of csrc/cc_pose_math.h with mpmath, and print them as C hex-float literals.

Three even/odd kernels, each a polynomial in z = x^2 fitted by interpolation at the Chebyshev nodes of the interval (within a small factor
of the minimax polynomial; one degree more than minimax would need) and then rounded to double:

    asin x = x + x z A(z)        z in [0, 1/4]        (|x| <= 1/2; acos x = pi/2 - asin x below 1/2, 2 asin sqrt((1 - x) / 2) above)
    sin  x = x + x z S(z)        z in [0, 0.62]       (x <= pi/4; (pi/4)^2 = 0.6169)
    cos  y = 1 - z/2 + z^2 C(z)  z in [0, 0.62]       (sin x = cos(pi/2 - x) above pi/4)

For each kernel the script prints, per degree, the largest relative error of the approximation with the ROUNDED coefficients evaluated
exactly, over a dense grid, as log2. The error stops falling near 2^-57 .. 2^-59, where the rounding of the leading coefficient to a
double sets it; the header uses the lowest degree that reaches that floor (A 13, S 6, C 5), 1/16 of the arithmetic's own rounding.

    python tools/pose_math_coeffs.py            # the table of errors per degree
    python tools/pose_math_coeffs.py --emit     # the chosen coefficients as C literals
"""
from __future__ import annotations

import sys

import mpmath as mp

mp.mp.dps = 90

KERNELS = {
    # name: (g(z), upper end of z, f(x), x -> approximation from the polynomial value p at z = x^2, chosen degree)
    "A": (lambda z: (mp.asin(mp.sqrt(z)) / mp.sqrt(z) - 1) / z, mp.mpf(1) / 4, mp.asin, lambda x, p: x + x * (x * x) * p, 13),
    "S": (lambda z: (mp.sin(mp.sqrt(z)) / mp.sqrt(z) - 1) / z, mp.mpf("0.62"), mp.sin, lambda x, p: x + x * (x * x) * p, 6),
    "C": (lambda z: (mp.cos(mp.sqrt(z)) - 1 + z / 2) / (z * z), mp.mpf("0.62"), mp.cos, lambda x, p: 1 - (x * x) / 2 + (x * x) ** 2 * p, 5),
}


def fit(g, b, degree):
    """Monomial coefficients (doubles, as mpf) of the interpolant of g at the degree + 1 Chebyshev nodes of [0, b]."""
    n = degree + 1
    nodes = [b / 2 * (1 + mp.cos(mp.pi * (2 * k + 1) / (2 * n))) for k in range(n)]
    V = mp.matrix(n, n)
    for i, z in enumerate(nodes):
        for j in range(n):
            V[i, j] = z ** j
    c = mp.lu_solve(V, mp.matrix([g(z) for z in nodes]))
    return [mp.mpf(float(c[j])) for j in range(n)]


def worst(coeffs, b, f, approx, grid=4000):
    w = mp.mpf(0)
    for k in range(1, grid + 1):
        x = mp.sqrt(b) * k / grid
        p = mp.polyval(coeffs[::-1], x * x)
        w = max(w, abs(approx(x, p) - f(x)) / abs(f(x)))
    return w


def main(argv):
    emit = "--emit" in argv
    for name, (g, b, f, approx, chosen) in KERNELS.items():
        if emit:
            c = fit(g, b, chosen)
            print(f"// {name}: degree {chosen} in z on [0, {mp.nstr(b, 4)}], error 2^{mp.nstr(mp.log(worst(c, b, f, approx), 2), 4)}")
            print("    " + ", ".join(float(v).hex() for v in c))
        else:
            for d in range(4, 19):
                c = fit(g, b, d)
                print(name, d, mp.nstr(mp.log(worst(c, b, f, approx, 600), 2), 5))
    if emit:
        hi = float(mp.pi / 2)
        lo = float(mp.pi / 2 - mp.mpf(hi))
        print("// pi/2 = hi + lo; pi/4")
        print("    " + ", ".join(v.hex() for v in (hi, lo, float(mp.pi / 4))))


if __name__ == "__main__":
    main(sys.argv[1:])

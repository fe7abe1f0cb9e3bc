"""Writes tests/golden/nipv_truth.json: the negative integrated posterior variance of two tiny
states at 40 significant digits (mpmath), by direct conditioning on [Xn; X_c].

    python tests/golden/make_nipv_truth.py

States: B = 2 outputs (RBF and Matern-5/2), n = 6 training rows, N = 5 integration points, d = 2,
noise 1e-2 (state 0) and 1e-4 (state 1); candidates with q = 1 and q = 2, one candidate point equal
to a training row and one equal to an integration point.  The inputs are the float64 values of the
three-digit decimals below, taken exactly; the values are stored as 40-digit strings.  Values
only."""
import json
import os

import mpmath as mp

mp.mp.dps = 60

XN = [[0.125, 0.875], [0.412, 0.237], [0.731, 0.642], [0.918, 0.105], [0.286, 0.553], [0.604, 0.951]]
P = [[0.250, 0.250], [0.750, 0.250], [0.500, 0.500], [0.250, 0.750], [0.750, 0.750]]
LS = [[0.450, 0.800], [0.350, 0.600]]
KINDS = [0, 3]
W = [0.5, 0.5]
YS = [1.300, 0.700]
CANDS = [
    [[0.333, 0.444]],                      # q = 1, generic
    [[0.731, 0.642]],                      # q = 1, equals training row 2
    [[0.500, 0.500]],                      # q = 1, equals integration point 2
    [[0.155, 0.322], [0.866, 0.577]],      # q = 2, generic
    [[0.412, 0.237], [0.250, 0.750]],      # q = 2, training row 1 and integration point 3
]
NOISES = [[0.010, 0.010], [0.0001, 0.0001]]


def k(x1, x2, ls, kind):
    d2 = sum(((mp.mpf(a) - mp.mpf(b)) / mp.mpf(l)) ** 2 for a, b, l in zip(x1, x2, ls))
    if kind == 0:
        return mp.exp(-d2 / 2)
    s = mp.sqrt(5 * d2)
    return (1 + s + mp.mpf(5) / 3 * d2) * mp.exp(-s)


def acq(xc, noise):
    total = mp.mpf(0)
    Z = XN + xc
    m = len(Z)
    for j, kind in enumerate(KINDS):
        K = mp.matrix(m, m)
        for a in range(m):
            for b in range(m):
                K[a, b] = k(Z[a], Z[b], LS[j], kind) + (mp.mpf(noise[j]) if a == b else 0)
        var_sum = mp.mpf(0)
        for p in P:
            kp = mp.matrix([k(z, p, LS[j], kind) for z in Z])
            sol = mp.lu_solve(K, kp)
            var_sum += 1 - sum(kp[a] * sol[a] for a in range(m))
        coef = (mp.mpf(W[j]) * mp.mpf(YS[j])) ** 2
        total -= coef * var_sum / len(P)
    return total


def main():
    states = []
    for noise in NOISES:
        states.append({"noise": noise, "acq": [mp.nstr(acq(c, noise), 40) for c in CANDS]})
    out = {"Xn": XN, "P": P, "ls": LS, "kinds": KINDS, "w": W, "ys": YS, "candidates": CANDS, "states": states,
           "digits": 40}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "nipv_truth.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

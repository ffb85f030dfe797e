"""Float64 references for the client-drift corrections (ffm_drift_correct, fairfedmed_amd/drift.py), written from the
formulas of DESIGN.md section 4.23 and of the papers, not from the module under test:

  FedProx   (Li et al. 2020):           g <- g + mu (p - anchor)            anchor: the weights at the start of the round
  SCAFFOLD  (Karimireddy et al. 2020):  g <- g + c - c_i
            option II without a learning rate: c_i' = mean of the raw gradients of the client's local steps,
            c <- c + sum over participants (c_i' - c_i) / N  (N: all clients), c_i <- c_i'

and the heterogeneous quadratics the behaviour tests train on.
"""
import numpy as np


def correct(g, p=None, anchor=None, mu=0.0, c_diff=None):
    """The corrected gradient in float64 (inputs of any float type)."""
    x = np.asarray(g, dtype=np.float64).copy()
    if anchor is not None:
        x += np.float64(np.float32(mu)) * (np.asarray(p, dtype=np.float64) - np.asarray(anchor, dtype=np.float64))
    if c_diff is not None:
        x += np.asarray(c_diff, dtype=np.float64)
    return x


def bound(g, p=None, anchor=None, mu=0.0, c_diff=None):
    """Per-element bound on |fp32 result - correct(...)|: four roundings (p - anchor, mu * d, g + t, x + c_diff) of at most 2^-24
    relative each, every intermediate bounded by |g| + |mu (p - anchor)| + |c_diff|  ->  2^-22 times that sum."""
    s = np.abs(np.asarray(g, dtype=np.float64))
    if anchor is not None:
        s = s + np.abs(np.float64(np.float32(mu)) * (np.asarray(p, dtype=np.float64) - np.asarray(anchor, dtype=np.float64)))
    if c_diff is not None:
        s = s + np.abs(np.asarray(c_diff, dtype=np.float64))
    return 2.0 ** -22 * s


class Scaffold:
    """The round protocol in float64: begin(i) -> c - c_i; step(raw) once per local step; end(i); finish(participants)."""

    def __init__(self, users, n):
        self.users = users
        self.c = np.zeros(n)
        self.c_i = np.zeros((users, n))
        self.new = {}
        self._sum, self._k = np.zeros(n), 0

    def begin(self, i):
        self._sum, self._k = np.zeros_like(self.c), 0
        return self.c - self.c_i[i]

    def step(self, raw):
        self._sum = self._sum + np.asarray(raw, dtype=np.float64)
        self._k += 1

    def end(self, i):
        if self._k > 0:
            self.new[i] = self._sum / self._k

    def finish(self, participants):
        for i in sorted(participants):
            if i in self.new:
                self.c = self.c + (self.new[i] - self.c_i[i]) / self.users
                self.c_i[i] = self.new[i]
        self.new = {}


def quadratics(clients=4, d=8, seed=0):
    """Client i's loss is 1/2 (x - b_i)^T A_i (x - b_i): first the A_i = diag(U(0.2, 2.0)), then the b_i ~ N(0, 1), from one
    generator, which is returned for whatever the caller draws next (the participants of a round)."""
    rng = np.random.default_rng(seed)
    A = np.stack([rng.uniform(0.2, 2.0, d) for _ in range(clients)])
    b = np.stack([rng.normal(0.0, 1.0, d) for _ in range(clients)])
    return A, b, rng


def pooled_optimum(A, b):
    """argmin of the equally weighted sum of the clients' losses (diagonal A_i): (sum A_i)^-1 sum A_i b_i."""
    return (A * b).sum(0) / A.sum(0)

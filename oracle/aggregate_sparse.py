"""CHECKER (test infrastructure, see oracle/__init__.py) of ``preprocess_aggregate`` / ``aggregate_neighbors`` at sizes
the dense checker (oracle/aggregate_torch.py: [N, N, 2E]) cannot reach: the same definition, this repository's own,
stated over a pair list.  Only tests import it.  float64 on the CPU.

* ``brute_pairs`` / ``brute_pairs_periodic``: the neighbour relation by testing every pair, in blocks of rows --
  an independent statement of what the grid walk of pigs_amd/csrc/aggregate.hip has to find.  Every pair comes with
  its q and with S = |a dx^2| + |2 b dx dy| + |c dy^2|, the scale of the roundings of q: a kernel that evaluates
  q in a format of unit roundoff u may decide a pair with |q - q_max| <= 8 u S either way (``classify``).
* ``aggregate``: out [N, L] from a pair list (I, J), differentiable by autograd with respect to all six arguments.
"""
import math

import torch

U = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
BAND_UNITS = 8.0
# (kx, ky) of image block k, the block order of pigs_periodic_images (include/pigs_amd.h)
SHIFTS = ((0, 0), (-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))


def _block_pairs(rows, means, conics, q_max, slack, extra=None):
    """Pairs (row r of ``rows``, column j of ``means`` / ``conics``) with q <= q_max + slack * S'.  A pair with
    q > q_max + 1 is never returned (no band is meant to be that wide); ``extra`` sees the others only."""
    dx = means[None, :, 0] - rows[:, None, 0]                    # mu_j - mu_i
    dy = means[None, :, 1] - rows[:, None, 1]
    a, b, c = conics[None, :, 0], conics[None, :, 1], conics[None, :, 2]
    q = a * dx * dx + 2 * b * dx * dy + c * dy * dy
    r, j = (q <= q_max + 1).nonzero(as_tuple=True)
    dx, dy, q = dx[r, j], dy[r, j], q[r, j]
    a, b, c = conics[j, 0], conics[j, 1], conics[j, 2]
    S = (a * dx * dx).abs() + (2 * b * dx * dy).abs() + (c * dy * dy).abs()
    if extra is not None:
        S = S + extra(j, dx, dy, a, b, c)
    keep = q <= q_max + slack * S
    return r[keep], j[keep], q[keep], S[keep]


def brute_pairs(means, conics, q_max, band_units=BAND_UNITS, block=512, u=U[torch.float32]):
    """Every pair (i, j) with q_ij = (mu_i - mu_j)^T C_j (mu_i - mu_j) <= q_max + band_units * u * S_ij, by testing
    all N^2 in blocks of ``block`` rows: (i, j, q, S), int64 / float64, ordered by (i, j).  ``means`` [N, 2] and
    ``conics`` [N, 3] are the inputs as the kernel saw them (already rounded), taken to float64 here."""
    means, conics = means.detach().double().cpu(), conics.detach().double().cpu().reshape(-1, 3)
    out = ([], [], [], [])
    for r0 in range(0, means.shape[0], block):
        r, j, q, S = _block_pairs(means[r0:r0 + block], means, conics, q_max, band_units * u)
        for lst, v in zip(out, (r + r0, j, q, S)):
            lst.append(v)
    return tuple(torch.cat(v) for v in out)


def periodic_images(means, conics, lo, period, wrap=True):
    """The 9N images of the wrapped centres in the block order of pigs_periodic_images: means [9N, 2], conics [9N, 3].
    ``wrap=False`` takes the centres as they are -- block 0 of pigs_periodic_images, which lies in the CLOSED box: a
    centre on lo + period is the same point of the torus as one on lo, but it meets its neighbours through other
    images k, and the lists name k."""
    m = means.detach().double().cpu()
    if wrap:
        m = lo + torch.remainder(m - lo, period)
    sh = torch.tensor(SHIFTS, dtype=torch.float64) * period
    return (m[None] + sh[:, None, :]).reshape(-1, 2), conics.detach().double().cpu().reshape(-1, 3).repeat(9, 1)


def brute_pairs_periodic(means, conics, q_max, lo, period, band_units=BAND_UNITS, block=512, u=U[torch.float32], wrap=True):
    """The same on the torus [lo, lo + period)^2: rows of block 0 against the 9N images, (i, j, k, q, S) ordered by
    (i, k, j).  The kernels take delta = (mu'_j - mu'_i) + s_k L: the difference is rounded (by at most u |mu'_j -
    mu'_i| per axis) before the shift makes it small, which moves q by up to |dq/d delta| times that, so S carries
    that term too (divided by band_units, so that band_units * u * S bounds the sum of both).  ``wrap``: see
    periodic_images."""
    means, conics = means.detach().double().cpu(), conics.detach().double().cpu().reshape(-1, 3)
    N = means.shape[0]
    m9, c9 = periodic_images(means, conics, lo, period, wrap)
    shift = (torch.tensor(SHIFTS, dtype=torch.float64) * period).repeat_interleave(N, 0)     # [9N, 2]

    def extra(j, dx, dy, a, b, c):
        ux, uy = (dx - shift[j, 0]).abs(), (dy - shift[j, 1]).abs()                          # |mu'_j - mu'_i|
        return (2 * (a * dx + b * dy).abs() * ux + 2 * (b * dx + c * dy).abs() * uy) / band_units

    out = ([], [], [], [])
    for r0 in range(0, N, block):
        r, j, q, S = _block_pairs(m9[r0:min(r0 + block, N)], m9, c9, q_max, band_units * u, extra if band_units > 0 else None)
        for lst, v in zip(out, (r + r0, j, q, S)):
            lst.append(v)
    i, col, q, S = (torch.cat(v) for v in out)
    return i, col % N, col // N, q, S


def classify(q, S, q_max, dtype, band_units=BAND_UNITS):
    """(sure_in, band) masks of pairs from brute_pairs for a kernel that works in ``dtype``; the rest is sure out."""
    w = band_units * U[dtype] * S
    sure_in = q <= q_max - w
    return sure_in, ~sure_in & (q <= q_max + w)


def aggregate(N, I, J, means, conics, features, transform, queries, keys, frequencies, distance_transform):
    """The definition of oracle/aggregate_torch.py over the pair list (I, J): row i = I[p] in [0, N) has neighbour
    J[p], an index into ``means`` / ``conics`` / ``features`` / ``keys`` (which may hold more than N rows: the 9N
    images, with the per-Gaussian arguments repeated); ``queries`` [N, K] and the centre of row i are rows i."""
    L, K, F = features.shape[1], queries.shape[1], frequencies.shape[0]
    E = 4 * F + 1
    if transform.shape != (L, L) or keys.shape[1] != K or distance_transform.shape != (L, 2 * E):
        raise ValueError(f"aggregate: expected transform [{L},{L}], keys [*,{K}], distance_transform [{L},{2 * E}]")
    P = I.shape[0]
    with torch.no_grad():
        delta = means[J] - means[I]                                           # mu_j - mu_i
        cj = conics.reshape(-1, 3)[J]
        dx, dy = delta[:, 0], delta[:, 1]
        g = torch.exp(-0.5 * (cj[:, 0] * dx * dx + 2 * cj[:, 1] * dx * dy + cj[:, 2] * dy * dy))
    s = (queries[I] * keys[J]).sum(-1) / math.sqrt(K)
    with torch.no_grad():
        top = torch.full((N,), -math.inf, dtype=s.dtype).scatter_reduce(0, I, s, "amax")
    w = torch.exp(s - top[I])
    attn = w / torch.zeros(N, dtype=s.dtype).index_add(0, I, w)[I]
    phase = delta[:, :, None] * frequencies                                   # [P, axis, F]
    emb = torch.stack((torch.sin(phase), torch.cos(phase)), dim=-1)           # [P, axis, F, sin|cos]
    emb = emb.permute(0, 2, 1, 3).reshape(P, 4 * F)                           # (k, axis, sin|cos) order
    emb = torch.cat((emb, torch.ones((P, 1), dtype=emb.dtype)), dim=-1)       # [P, E]
    emb2 = torch.cat((emb, g[:, None] * emb), dim=-1)                         # [P, 2E]
    fbar = torch.zeros((N, L), dtype=s.dtype).index_add(0, I, attn[:, None] * features[J])
    ebar = torch.zeros((N, 2 * E), dtype=s.dtype).index_add(0, I, attn[:, None] * emb2)
    return fbar @ transform.t() + ebar @ distance_transform.t()

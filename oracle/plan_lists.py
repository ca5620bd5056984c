"""The binned path's tile lists against a brute-force statement of their contract (TEST INFRASTRUCTURE, see
oracle/__init__.py; CPU, numpy, float64).

pigs_amd/csrc/plan.h: "a (point, Gaussian) pair is evaluated iff the Gaussian's ellipse q <= q_max reaches the
bounding box of the point's 16-point group", by an exact ellipse / rectangle test.  Here that sentence is restated
without the kernel's formula (:func:`min_q_rect`), the grouping of the points is read back from a samples workspace or
restated for the index-tiled order (:func:`groups_of`), and a plan's headers, tile lists, group lists and record ranges
are held against it entry by entry (:func:`check_plan`).  :func:`pair_mask` says which pairs the sampling kernels then
evaluate, per tile mode and direction, for a masked dense oracle (oracle/dense_numpy.py, ``pair_mask=``).

The float32 kernel and the float64 oracle may disagree about a pair whose minimum q lies within ``DELTA`` (relative) of
a cut-off: the BAND.  Every two-sided condition leaves the band open, and every caller counts the band pairs.
"""
import numpy as np

# plan.h: tile header word 0 = count | mode << 30; tile-list entry = sorted index | wide mask << 24 | narrow mask << 28
LIST, RANGES, GROUPS, POINTS = 0, 1, 2, 3
MODE_NAMES = ("list", "ranges", "groups", "points")
MODE_SHIFT, HDR_WORDS = 30, 8
COUNT_MASK = (1 << MODE_SHIFT) - 1
IDX_BITS, WIDE_SHIFT, NARROW_SHIFT = 24, 24, 28
IDX_MASK = (1 << IDX_BITS) - 1
TILE_POINTS, GROUP_POINTS = 64, 16

# Half-width of the band, relative in q.  Measured by tests/test_plan_lists.py::test_delta_is_four_times_the_measured_
# disagreement: grid_walk.h's closed form in numpy float32 (true division, no v_rcp_f32) against the same in float64
# disagrees by at most 4.45e-6 relative over the pairs with a minimum q in [q_max / 2, 2 q_max] of every scene of
# tests/test_plan_lists_gpu.py (256 000 pairs) against the boxes of 16 cell-sorted points.  The worst pair belongs to
# scene G of tests/test_binned_matrix_gpu.py (random_gaussians' correlations tanh(N(0, 0.7)): b / sqrt(a c) = -0.984);
# the other scenes stay below 1.9e-6.  DELTA is four times the worst, rounded up: the factor covers v_rcp_f32's 1 ulp
# and the device's FMA contraction, neither of which the emulation has.
DELTA = 2e-5


def decode_headers(hdr):
    """hdr [tiles, 8] uint32 -> mode [tiles], count [tiles], group list lengths [tiles, 4] (int64)"""
    hdr = np.asarray(hdr).astype(np.int64).reshape(-1, HDR_WORDS)
    return hdr[:, 0] >> MODE_SHIFT, hdr[:, 0] & COUNT_MASK, hdr[:, 1:5]


def decode_entries(entries):
    """tile-list entries -> sorted Gaussian index, wide group mask, narrow group mask"""
    e = np.asarray(entries).astype(np.int64)
    return e & IDX_MASK, (e >> WIDE_SHIFT) & 15, (e >> NARROW_SHIFT) & 15


# ------------------------------------------------------------------------------------------
# which 16 points form a group
# ------------------------------------------------------------------------------------------
def lattice_tiles(ntx, nty):
    """The index-tiled order (plan.h, SampleParams::lat) as a walk: [tiles, 2] = (tx, ty) of the 8 x 8 index patch at
    every position.  Pair-rows of tiles are taken alternately left to right and right to left, inside a pair-row column
    by column (lower tile first); an odd nty leaves one last row that continues the serpentine."""
    order = []
    for pr in range(nty // 2):
        cols = range(ntx) if pr % 2 == 0 else range(ntx - 1, -1, -1)
        for tx in cols:
            order += [(tx, 2 * pr), (tx, 2 * pr + 1)]
    if nty % 2:
        cols = range(ntx) if (nty // 2) % 2 == 0 else range(ntx - 1, -1, -1)
        order += [(tx, nty - 1) for tx in cols]
    return np.asarray(order, dtype=np.int64).reshape(-1, 2)


def groups_of(M, lat=(0, 0), m_words=None):
    """[tiles, 4, 16] indices into the caller's point array, -1 where a ragged last tile has no point.
    ``lat`` = {rf, rs} of the samples workspace: non-zero for an rf x rs lattice in row order taken in index-tiled
    order (tile = 8 x 8 index patch, group g = its 4 x 4 patch (g & 1, g >> 1), rows of four inside a group);
    {0, 0}: the points were sorted, ``m_words`` [M] are the sorted points' indices in the caller's array."""
    rf, rs = int(lat[0]), int(lat[1])
    tiles = -(-M // TILE_POINTS)
    if rf:
        assert rf % 8 == 0 and rs % 8 == 0 and rf * rs == M, (rf, rs, M)
        txy = lattice_tiles(rf // 8, rs // 8)
        g, i = np.arange(4)[:, None], np.arange(16)[None, :]
        col = txy[:, 0, None, None] * 8 + (g & 1) * 4 + (i & 3)
        row = txy[:, 1, None, None] * 8 + (g >> 1) * 4 + (i >> 2)
        return row * rf + col
    m = np.full(tiles * TILE_POINTS, -1, dtype=np.int64)
    m[:M] = np.asarray(m_words).astype(np.int64)
    return m.reshape(tiles, 4, GROUP_POINTS)


def group_boxes(points, groups):
    """[tiles, 4, 4] = {min x, min y, max x, max y} of every group; a group without a point has the inverted box
    {inf, inf, -inf, -inf}."""
    points = np.asarray(points, dtype=np.float64)
    have = groups >= 0
    p = points[np.where(have, groups, 0)]
    lo = np.where(have[..., None], p, np.inf).min(2)
    hi = np.where(have[..., None], p, -np.inf).max(2)
    return np.concatenate((lo, hi), -1)


def tile_boxes(gboxes):
    return np.concatenate((gboxes[:, :, :2].min(1), gboxes[:, :, 2:].max(1)), -1)


# ------------------------------------------------------------------------------------------
# the minimum of q over a rectangle
# ------------------------------------------------------------------------------------------
def _min_q(l, r, bt, tp, a, b, c):
    """the rectangle [l, r] x [bt, tp] in coordinates relative to the centre (broadcastable arrays)"""
    def vertical(dx):          # the edge at horizontal offset dx; the parabola in dy has its vertex at -b dx / c
        dy = np.minimum(np.maximum(-b * dx / c, bt), tp)
        return a * dx * dx + 2 * b * dx * dy + c * dy * dy

    def horizontal(dy):
        dx = np.minimum(np.maximum(-b * dy / a, l), r)
        return a * dx * dx + 2 * b * dx * dy + c * dy * dy

    with np.errstate(invalid="ignore", over="ignore"):
        q = np.minimum(np.minimum(vertical(l), vertical(r)), np.minimum(horizontal(bt), horizontal(tp)))
        q = np.where((l <= 0) & (r >= 0) & (bt <= 0) & (tp >= 0), 0.0, q)
        return np.where(l > r, np.inf, q)


def min_q_rect(means, conics, boxes, chunk_pairs=1 << 21, paired=False):
    """[boxes, N]: the minimum over the rectangle {x0, y0, x1, y1} of q(s) = (s - mu)^T C (s - mu), C = flat conic
    {a, b, c}.  0 when the centre lies inside; otherwise q is convex and its minimum lies on the boundary: the smallest
    of four edge minima, each a 1-D parabola whose free coordinate is clamped to the edge.  An inverted box (a group
    without a point) gives +inf.  Chunked over boxes.  ``paired``: box k against Gaussian k alone, [N]."""
    means, conics = np.asarray(means, dtype=np.float64), np.asarray(conics, dtype=np.float64)
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    mx, my = means[:, 0], means[:, 1]
    a, b, c = conics[:, 0], conics[:, 1], conics[:, 2]
    if paired:
        return _min_q(boxes[:, 0] - mx, boxes[:, 2] - mx, boxes[:, 1] - my, boxes[:, 3] - my, a, b, c)
    B, N = boxes.shape[0], means.shape[0]
    out = np.empty((B, N))
    step = max(1, chunk_pairs // max(N, 1))
    for s in range(0, B, step):
        bx = boxes[s:s + step]
        out[s:s + step] = _min_q(bx[:, 0, None] - mx, bx[:, 2, None] - mx, bx[:, 1, None] - my, bx[:, 3, None] - my, a, b, c)
    return out


def pair_q(means, conics, points):
    """[M, N]: q of every (point, Gaussian) pair."""
    means, conics = np.asarray(means, dtype=np.float64), np.asarray(conics, dtype=np.float64)
    points = np.asarray(points, dtype=np.float64)
    dx, dy = points[:, 0, None] - means[:, 0], points[:, 1, None] - means[:, 1]
    return conics[:, 0] * dx * dx + 2 * conics[:, 1] * dx * dy + conics[:, 2] * dy * dy


def closed_form_min_q(means, conics, boxes, dtype):
    """grid_walk.h's ellipse_min_q_rect restated in numpy at ``dtype``, operation by operation (true division where the
    kernel takes v_rcp_f32, no contraction): [boxes, N].  For measuring DELTA only; the checker uses min_q_rect."""
    f = np.dtype(dtype).type
    means, conics, boxes = (np.asarray(x).astype(dtype) for x in (means, conics, boxes))
    ex, ey = means[:, 0], means[:, 1]
    a, b, c = conics[:, 0], conics[:, 1], conics[:, 2]
    nb_c, nb_a = -b / c, -b / a
    l, r = boxes[:, 0, None] - ex, boxes[:, 2, None] - ex
    bt, tp = boxes[:, 1, None] - ey, boxes[:, 3, None] - ey
    med3 = lambda v, lo, hi: np.minimum(np.maximum(v, lo), hi)
    xe, ye = med3(f(0), l, r), med3(f(0), bt, tp)
    ys, xs = med3(nb_c * xe, bt, tp), med3(nb_a * ye, l, r)
    q1 = a * xe * xe + (f(2) * b * xe + c * ys) * ys
    q2 = c * ye * ye + (f(2) * b * ye + a * xs) * xs
    q = np.minimum(q1, q2)
    assert q.dtype == np.dtype(dtype)
    return q


# ------------------------------------------------------------------------------------------
# the checker
# ------------------------------------------------------------------------------------------
def _duplicates(idx):
    u, n = np.unique(idx, return_counts=True)
    return u[n > 1]


def check_plan(hdr, tlist, glist, g2o, means, conics, points, groups, q_f, q_b, strips=False, forward_only=False,
               delta=DELTA, tiles=None, stats=None):
    """A plan's lists against the contract.  Returns the findings, a list of (what, tile, group, Gaussian): the
    Gaussian is its index in the CALLER's array, -1 where a finding has no group / Gaussian (or the index is broken).

    hdr [tiles, 8], tlist [tiles, cap], glist [tiles, 4, cap], g2o [N] as the workspace holds them; means [N, 2],
    conics [N, 3], points [M, 2]: the float32-rounded inputs in float64; groups: :func:`groups_of`; q_f <= q_b: the
    plan's narrow and wide cut-off.  ``strips``: the build kept the caller's order (PlanParams::strips) -- g2o is then
    the identity (plan_build.h, gauss_pack_part: gauss_scatter_one(a, i, i)).  ``forward_only``: one cut-off, group
    lists only; the tile list is not read.  ``tiles``: check these tiles only.  ``stats`` (a dict) receives: tiles per
    mode, the longest list, the must-have and the band pairs, and for RANGES tiles the Gaussians their ranges hold and
    those they need.

    What the code deliberately does not keep of plan.h's sentence, and is therefore not a finding: a GROUPS tile's
    group lists hold the WIDE set (the forward evaluates a few pairs beyond q_f there); RANGES are coarse by design
    (only the lower condition)."""
    means, conics = np.asarray(means, dtype=np.float64), np.asarray(conics, dtype=np.float64)
    N = means.shape[0]
    mode, count, ng = decode_headers(hdr)
    ntiles, cap = len(mode), tlist.shape[1]
    tlist, glist = np.asarray(tlist).astype(np.int64), np.asarray(glist).astype(np.int64).reshape(ntiles, 4, cap)
    hdr = np.asarray(hdr).astype(np.int64).reshape(ntiles, HDR_WORDS)
    g2o = np.asarray(g2o).astype(np.int64)
    found = []
    st = {"tiles": [0, 0, 0, 0], "longest": 0, "must": 0, "band": 0, "ranges_held": 0, "ranges_needed": 0}
    assert groups.shape == (ntiles, 4, GROUP_POINTS) and q_b >= q_f
    if forward_only:
        q_b = q_f

    # ---- per plan
    if not (len(g2o) == N and (np.sort(g2o) == np.arange(N)).all()):
        found.append(("g2o is no permutation of 0..N-1", -1, -1, -1))
        return found
    if strips and not (g2o == np.arange(N)).all():
        found.append(("strips: g2o is not the identity", -1, -1, -1))

    gboxes = group_boxes(points, groups)
    tboxes = tile_boxes(gboxes)
    todo = np.arange(ntiles) if tiles is None else np.asarray(sorted(set(int(t) for t in tiles)))
    step = max(1, (1 << 21) // (4 * max(N, 1)))

    def two_sided(t, g, have, q, cut, what):
        """have [N] bool by caller index: every must-have pair, no pair beyond the band"""
        st["must"] += int((q <= cut * (1 - delta)).sum())
        st["band"] += int((np.abs(q - cut) <= cut * delta).sum())
        for n in np.flatnonzero(~have & (q <= cut * (1 - delta))):
            found.append((f"missing from the {what} set (min q {q[n]:.6g} <= {cut:g})", t, g, int(n)))
        for n in np.flatnonzero(have & (q > cut * (1 + delta))):
            found.append((f"in the {what} set without reaching the group (min q {q[n]:.6g} > {cut:g})", t, g, int(n)))

    def group_list(t, g):
        """group list g of tile t as sorted indices, or None when it is broken"""
        n = int(ng[t, g])
        if n > cap:
            found.append((f"group list of {n} entries in a slab of {cap}", t, g, -1))
            return None
        gl = glist[t, g, :n]
        if (gl >= N).any() or (gl < 0).any():
            found.append(("group list entry beyond N", t, g, -1))
            return None
        for j in _duplicates(gl):
            found.append(("duplicate in the group list", t, g, int(g2o[j])))
        st["longest"] = max(st["longest"], n)
        return gl

    for s in range(0, len(todo), step):
        chunk = todo[s:s + step]
        qmin = min_q_rect(means, conics, gboxes[chunk].reshape(-1, 4)).reshape(len(chunk), 4, N)
        for k, t in enumerate(chunk):
            t = int(t)
            md = int(mode[t])
            st["tiles"][md] += 1
            empty = gboxes[t, :, 0] > gboxes[t, :, 2]
            if md == POINTS:
                if list(hdr[t, :5]) != [POINTS << MODE_SHIFT, 0, 0, 0, 0]:
                    found.append(("POINTS tile whose header words 0..4 are not {mode << 30, 0, 0, 0, 0}", t, -1, -1))
                continue
            if md == RANGES:
                cnt = int(count[t])
                if cnt < 1 or 2 * cnt > cap:
                    found.append((f"RANGES tile with {cnt} ranges in a slab of {cap}", t, -1, -1))
                    continue
                first, length = tlist[t, 0:2 * cnt:2], tlist[t, 1:2 * cnt:2]
                if (first < 0).any() or (length < 0).any() or (first + length > N).any():
                    found.append(("range outside [0, N]", t, -1, -1))
                    continue
                held = np.zeros(N, dtype=np.int64)
                for f_, l_ in zip(first, length):
                    held[f_:f_ + l_] += 1
                for j in np.flatnonzero(held > 1):
                    found.append(("two ranges overlap", t, -1, int(g2o[j])))
                have = np.zeros(N, dtype=bool)
                have[g2o[held > 0]] = True
                cut = max(q_f, q_b)
                q = min_q_rect(means, conics, tboxes[t:t + 1])[0]
                need = q <= cut * (1 - delta)
                st["must"] += int(need.sum())
                st["band"] += int((np.abs(q - cut) <= cut * delta).sum())
                st["ranges_held"] += int(have.sum())
                st["ranges_needed"] += int(need.sum())
                for n in np.flatnonzero(need & ~have):
                    found.append((f"no range holds it (min q over the tile {q[n]:.6g} <= {cut:g})", t, -1, int(n)))
                continue
            if md == GROUPS or forward_only:
                if md == LIST and count[t] != 0:
                    found.append(("forward-only plan: LIST tile with a tile list", t, -1, -1))
                if md == GROUPS and forward_only:
                    found.append(("forward-only plan: GROUPS tile", t, -1, -1))
                for g in range(4):
                    gl = group_list(t, g)
                    if gl is None:
                        continue
                    have = np.zeros(N, dtype=bool)
                    have[g2o[gl]] = True
                    if empty[g] and len(gl):
                        found.append(("a group without a point has a list", t, g, -1))
                    two_sided(t, g, have, qmin[k, g], q_b, "wide" if md == GROUPS else "forward")
                continue
            # ---- LIST
            cnt = int(count[t])
            if cnt > cap:
                found.append((f"tile list of {cnt} entries in a slab of {cap}", t, -1, -1))
                continue
            idx, wide, narrow = decode_entries(tlist[t, :cnt])
            if (idx >= N).any():
                found.append(("tile list entry beyond N", t, -1, -1))
                continue
            st["longest"] = max(st["longest"], cnt)
            orig = g2o[idx]
            for j in _duplicates(idx):
                found.append(("duplicate in the tile list", t, -1, int(g2o[j])))
            for e in np.flatnonzero(narrow & ~wide):
                g = int(np.flatnonzero([(narrow[e] & ~wide[e]) >> b & 1 for b in range(4)])[0])
                found.append(("narrow bit without its wide bit", t, g, int(orig[e])))
            for e in np.flatnonzero(wide == 0):
                found.append(("tile list entry with an empty wide mask", t, -1, int(orig[e])))
            for g in range(4):
                wbit, nbit = (wide >> g & 1) == 1, (narrow >> g & 1) == 1
                if empty[g] and (wbit.any() or nbit.any() or ng[t, g] != 0):
                    found.append(("a group without a point has a bit or a list", t, g, -1))
                for bit, cut, what in ((wbit, q_b, "wide"), (nbit, q_f, "narrow")):
                    have = np.zeros(N, dtype=bool)
                    have[orig[bit]] = True
                    two_sided(t, g, have, qmin[k, g], cut, what)
                gl = group_list(t, g)
                if gl is None:
                    continue
                for j in np.setdiff1d(idx[nbit], gl):
                    found.append(("narrow bit without an entry in the group list", t, g, int(g2o[j])))
                for j in np.setdiff1d(gl, idx[nbit]):
                    found.append(("group list entry without its narrow bit in the tile list", t, g, int(g2o[j])))
    if stats is not None:
        stats.update(st)
    return found


# ------------------------------------------------------------------------------------------
# which pairs the sampling kernels evaluate
# ------------------------------------------------------------------------------------------
def pair_mask(mode, groups, means, conics, points, q_f, q_b, backward=False, wide=False, delta=DELTA):
    """([M, N] bool, [M, N] bool): the pairs a plan's sampling kernels evaluate, and the band pairs (within ``delta`` of
    the cut-off that decides them: either answer is right).  ``mode`` [tiles]: the tiles' mode words.  ``backward``:
    the backward launch; ``wide``: the INSTANTIATION that runs it takes gradients of order 2, order 3 or the trace (WIDE
    in plan_backward.h), so it reads the wide masks.  A request runs its covering instantiation (launch.h,
    covering_mask_of): gradients at orders (0, 1) run the (0, 1, 2) kernel, wide; only order 0 or order 1 alone is narrow.

      LIST    forward: the group's narrow list (q_f); backward: the wide mask (q_b) when ``wide``, the narrow otherwise
      GROUPS  the group lists hold the wide set: q_b in both directions
      RANGES  the ranges' records are tested against the group boxes: q_f forward, q_b / q_f backward as for LIST
      POINTS  the pair's own q(m, n) against the same cut-offs
    A forward-only plan passes q_b = q_f."""
    points = np.asarray(points, dtype=np.float64)
    M, N = points.shape[0], np.asarray(means).shape[0]
    qmin = min_q_rect(means, conics, group_boxes(points, groups).reshape(-1, 4)).reshape(len(mode), 4, N)
    mask, band = np.zeros((M, N), dtype=bool), np.zeros((M, N), dtype=bool)
    for t, md in enumerate(np.asarray(mode).astype(np.int64)):
        cut = q_b if md == GROUPS or (backward and wide) else q_f
        for g in range(4):
            mem = groups[t, g][groups[t, g] >= 0]
            if not len(mem):
                continue
            q = pair_q(means, conics, points[mem]) if md == POINTS else np.broadcast_to(qmin[t, g], (len(mem), N))
            mask[mem] = q <= cut
            band[mem] = np.abs(q - cut) <= cut * delta
    return mask, band

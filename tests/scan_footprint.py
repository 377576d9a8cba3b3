"""Where one non-finite operand element of the selective scan may show in the outputs: a dependency rule written as set
arithmetic (no floating point), the plants a GPU launch carries, and the checker that holds a kernel's outputs to the rule.
Plain torch, no GPU needed; tests/test_scan_fp64_cpu.py anchors the rule on the fp64 reference and on a literal loop.
Non-finite VALUES are data, not addresses: nothing here makes a kernel read or write outside memory the test owns.

The rule (scan order s of a row; a reversed row has s = L - 1 - t).  A product is hit when a factor is hit (0 * NaN and
0 * inf are NaN), a sum when a term is.  With dl = softplus(delta + bias), a = exp(dl A), w = dl u B:

    x_s   = a_s x_{s-1} + w_s           hit: a or w hit at some s'' <= s  (x_{-1} = 0 is a state like any other: a_0 x_{-1})
    lam_s = g_s C_s + a_{s+1} lam_{s+1} hit: g or C hit at some s'' >= s, or a hit at some s'' > s
    out_s    = sum_n C x + D u          du_s = dl_s sum_n B lam + D g_s
    ddelta_s = (u_s sum_n B lam + sum_n A a_s x_{s-1} lam_s) sigmoid_s
    dA[n]    = sum_{b,s} dl a x_{s-1} lam       dB_s[n] = sum_rows dl u lam        dC_s[n] = sum_rows g x
    dD = sum_{b,s} g u                  ddelta_bias = sum_{b,s} ddelta

so ``out`` runs from the plant toward the end of the scan (the start of the memory row when the row is reversed) and the
adjoint quantities the other way; dA / dD / ddelta_bias of a row are hit whenever a term is; dB / dC over the plant's
(batch, group) only; a shared u / dout row feeds every group that reads it.  One value matters to the SET: delta = +inf
gives dl = +inf but a = exp(-inf) = 0 and sigmoid = 1, both finite (A < 0 on every regime), so the decay and the
softplus derivative carry nothing -- lam before the plant, and ddelta AT the plant, stay finite.  They stay finite but do
not keep the unplanted problem's VALUES (the adjoint no longer crosses the plant): the finite twin of such a launch is
the problem with DECAYED in the plant's place, whose a underflows to exactly 0 in fp64 and in fp32 and whose sigmoid is
1 -- outside the cones it equals the planted problem term by term, and it has a bound."""
from __future__ import annotations

import dataclasses

import torch

from tests import scan_fp64_ref as R

NAN, INF = float("nan"), float("inf")
DECAYED = 1.0e6              # a delta whose decay exp(delta A) is exactly 0 for |A| >= 1e-3 (fp64 underflows below -745)
SEQ_OPERANDS = ("u", "delta", "B", "C", "dout")
ROW_OPERANDS = ("A", "D", "delta_bias")
ARG_INDEX = {"u": 0, "delta": 1, "A": 2, "B": 3, "C": 4, "D": 5, "delta_bias": 6, "dout": 7}
SEQ_OUTPUTS = ("out", "du", "ddelta", "dB", "dC")
# the five outputs with a sequence axis that an operand reaches at all (u does not enter du, dout not out, B not dB, C not dC, D neither)
REACHES = {"u": ("out", "ddelta", "dB", "dC"), "delta": ("out", "du", "ddelta", "dB", "dC"),
           "B": ("out", "du", "ddelta", "dC"), "C": ("out", "du", "ddelta", "dB"), "dout": ("du", "ddelta", "dB", "dC"),
           "A": ("out", "du", "ddelta", "dB", "dC"), "D": ("out", "du"), "delta_bias": ("out", "du", "ddelta", "dB", "dC")}


def reached(plant, dims, rev_mask=0, u_gshift=0, dout_gshift=0):
    """the outputs of REACHES in which the plant's cone is not empty: all of them, but for delta = +inf at the LAST scan
    position of its row, whose ddelta cone is empty (ddelta at the plant stays finite and nothing comes after it)"""
    names = REACHES[plant.operand]
    if plant.operand == "delta" and plant.value == INF:
        (_, _, _, rev, t, _), = rows_of(plant, dims, rev_mask, u_gshift, dout_gshift)
        if t == (0 if rev else dims[2] - 1):
            names = tuple(n for n in names if n != "ddelta")
    return names


@dataclasses.dataclass(frozen=True)
class Plant:
    operand: str                 # one of ARG_INDEX
    index: tuple                 # in the operand's own layout; the last entry of a SEQ operand is the memory position
    value: float = NAN           # NAN or INF


def _prefix(m):                  # exists s'' <= s
    return m.cumsum(-1) > 0


def _suffix(m):                  # exists s'' >= s
    return m.flip(-1).cumsum(-1).flip(-1) > 0


def _prev(m):                    # m_{s-1}, False at the first position
    out = torch.zeros_like(m)
    out[..., 1:] = m[..., :-1]
    return out


def _next(m):                    # m_{s+1}, False at the last position
    out = torch.zeros_like(m)
    out[..., :-1] = m[..., 1:]
    return out


def row_pattern(operand, s, n, value, N, L, softplus=True):
    """the hit sets of ONE row in scan order for a plant at scan position ``s`` (sequence operands) and state ``n`` (A, B,
    C): out, du, ddelta (L,), dB, dC terms (N, L), dA (N,), dD, ddelta_bias (bool)"""
    z = lambda *sh: torch.zeros(*sh, dtype=torch.bool)
    u_h, g_h, dl_h, sig_h, a_h, B_h, C_h, A_h, D_h = z(L), z(L), z(L), z(L), z(N, L), z(N, L), z(N, L), z(N), False
    if operand == "u":
        u_h[s] = True
    elif operand == "dout":
        g_h[s] = True
    elif operand == "delta":
        dl_h[s] = True
        if value != value:                                   # NaN; +inf leaves a = 0 and sigmoid = 1
            a_h[:, s] = True
            sig_h[s] = True
    elif operand == "B":
        B_h[n, s] = True
    elif operand == "C":
        C_h[n, s] = True
    elif operand == "A":
        A_h[n] = True
        a_h[n] = True
    elif operand == "D":
        D_h = True
    elif operand == "delta_bias":
        dl_h[:] = True
        a_h[:] = True
        sig_h[:] = True
    else:
        raise ValueError(operand)
    x_h = _prefix(dl_h | u_h | B_h | a_h)
    lam_h = _suffix(g_h | C_h) | _next(_suffix(a_h))
    sB = (B_h | lam_h).any(0)
    ax = a_h | _prev(x_h)
    out = (C_h | x_h).any(0) | u_h | D_h
    du = dl_h | sB | g_h | D_h
    ddelta = u_h | sB | (A_h[:, None] | ax | lam_h).any(0)
    if softplus:
        ddelta = ddelta | sig_h
    return {"out": out, "du": du, "ddelta": ddelta, "dA": (dl_h | ax | lam_h).any(-1), "dB": dl_h | u_h | lam_h,
            "dC": g_h | x_h, "dD": bool((g_h | u_h).any()), "ddelta_bias": bool(ddelta.any())}


def rows_of(plant, dims, rev_mask=0, u_gshift=0, dout_gshift=0):
    """[(batch images, rows (a slice), group, reversed, memory position or None, state or None)] of the rows a plant feeds"""
    batch, KD, L, N, G = dims
    rows = KD // G
    op, ix = plant.operand, plant.index
    rev = lambda g: bool((rev_mask >> g) & 1)
    every = list(range(batch))
    if op in ("u", "dout"):
        sh = u_gshift if op == "u" else dout_gshift
        b, j, t = ix
        return [([b], slice(g * rows + j % rows, g * rows + j % rows + 1), g, rev(g), t, None) for g in range(G) if (g >> sh) == j // rows]
    if op == "delta":
        b, r, t = ix
        return [([b], slice(r, r + 1), r // rows, rev(r // rows), t, None)]
    if op in ("B", "C"):
        b, g, n, t = ix
        return [([b], slice(g * rows, (g + 1) * rows), g, rev(g), t, n)]
    if op == "A":
        r, n = ix
        return [(every, slice(r, r + 1), r // rows, rev(r // rows), None, n)]
    (r,) = ix
    return [(every, slice(r, r + 1), r // rows, rev(r // rows), None, None)]


def empty_masks(dims):
    batch, KD, L, N, G = dims
    m = {"out": torch.zeros(batch, KD, L, dtype=torch.bool), "dA": torch.zeros(KD, N, dtype=torch.bool),
         "dB": torch.zeros(batch, G, N, L, dtype=torch.bool), "dD": torch.zeros(KD, dtype=torch.bool)}
    m["du"], m["ddelta"], m["dC"], m["ddelta_bias"] = m["out"].clone(), m["out"].clone(), m["dB"].clone(), m["dD"].clone()
    return m


def footprint(plant, dims, rev_mask=0, u_gshift=0, dout_gshift=0, softplus=True, into=None):
    """name -> bool mask (CPU, the output's own layout) of the elements of the eight OUTPUTS that depend on the plant.
    ``into``: masks of earlier plants to add this cone to; returns (overlap, sizes) instead -- whether the cone meets what
    ``into`` already held, and name -> number of elements of the cone (the outputs in which it is not empty)"""
    batch, KD, L, N, G = dims
    m = into if into is not None else empty_masks(dims)
    overlap, names = False, {}

    def add(t, p, k):
        nonlocal overlap
        if bool(torch.as_tensor(p).any()):
            if into is not None:
                overlap = overlap or bool((t & p).any())
            names[k] = names.get(k, 0) + int((torch.zeros_like(t) | p).sum())
        t |= p
    cache = {}
    for bs, r, g, rev, t, n in rows_of(plant, dims, rev_mask, u_gshift, dout_gshift):
        key = (rev, t, n)
        if key not in cache:
            s = None if t is None else (L - 1 - t if rev else t)
            p = row_pattern(plant.operand, s, n, plant.value, N, L, softplus)
            cache[key] = {k: (v.flip(-1) if rev and k in ("out", "du", "ddelta", "dB", "dC") else v) for k, v in p.items()}
        p = cache[key]
        for b in bs:
            for k in ("out", "du", "ddelta"):
                add(m[k][b, r], p[k], k)
            add(m["dB"][b, g], p["dB"], "dB")
            add(m["dC"][b, g], p["dC"], "dC")
        add(m["dA"][r], p["dA"], "dA")
        add(m["dD"][r], p["dD"], "dD")
        add(m["ddelta_bias"][r], p["ddelta_bias"], "ddelta_bias")
    return m if into is None else (overlap, names)


def own(plant, dims, tile, rev_mask=0, u_gshift=0, dout_gshift=0, only_rev=None, into=None):
    """name -> bool mask of where a KERNEL may deviate from the rule at all (and then only through the table of the GPU
    test): the plant's own rows for out / du / ddelta / dA / dD / ddelta_bias, the plant's own (batch, group) and its own
    ``tile`` of memory positions for dB / dC.  A plant in A, D or delta_bias has no position and reaches every batch
    image; the one tile where its row differs from any other is the ragged one that holds the LAST scan position (the
    kernels pad it to a full tile), so that tile of its group stands for "its own".  ``only_rev``: the rows of that
    direction only; ``into``: masks to add to"""
    batch, KD, L, N, G = dims
    m = into if into is not None else empty_masks(dims)
    for bs, r, g, rev, t, n in rows_of(plant, dims, rev_mask, u_gshift, dout_gshift):
        if only_rev is not None and rev != only_rev:
            continue
        for b in bs:
            for k in ("out", "du", "ddelta"):
                m[k][b, r] = True
            t0 = (t if t is not None else (0 if rev else L - 1)) // tile * tile
            m["dB"][b, g, :, t0:t0 + tile] = True
            m["dC"][b, g, :, t0:t0 + tile] = True
        m["dA"][r] = True
        m["dD"][r] = True
        m["ddelta_bias"][r] = True
    return m


def union(masks):
    out = {k: torch.zeros_like(v) for k, v in masks[0].items()}
    for m in masks:
        for k, v in m.items():
            out[k] |= v
    return out


def disjoint(masks):
    """no element belongs to the cones of two plants"""
    count = {k: torch.zeros(v.shape, dtype=torch.int32) for k, v in masks[0].items()}
    for m in masks:
        for k, v in m.items():
            count[k] += v
    return all(int(c.max()) <= 1 for c in count.values())


def plant_into(args, plants):
    """the operands with the plants written in (clones of the planted tensors only)"""
    args = list(args)
    done = set()
    for p in plants:
        i = ARG_INDEX[p.operand]
        if i not in done:
            args[i] = args[i].clone()
            done.add(i)
        args[i][p.index] = p.value
    return args


def non_finite_sets(outputs):
    return {k: ~torch.isfinite(v.detach().double()).cpu() for k, v in outputs.items() if v is not None}


def check(got, cones, owns, ref, S, excused=None):
    """``got`` (name -> tensor) against the rule: returns (failures, deviations).  Outside the union of cones an element
    must be finite and inside the fp64 bound of the UNPLANTED problem (ref, S); inside a cone it must be non-finite -- a
    finite one is a lost NaN and never excused.  A non-finite element outside the cones is a deviation: a failure when it
    lies outside ``owns`` (another row, batch image, group or tile: never excused) or outside ``excused`` (name -> mask,
    the part of ``owns`` that the caller's table covers; None: nothing), counted in ``deviations[name]`` otherwise."""
    failures, deviations = [], {}
    for name, t in got.items():
        if t is None:
            continue
        dev = t.device
        g = t.detach().to(torch.float64)
        cone, mine = cones[name].to(dev), owns[name].to(dev)
        table = excused[name].to(dev) & mine if excused and name in excused else torch.zeros_like(mine)
        bad = ~torch.isfinite(g)
        lost = cone & ~bad
        if bool(lost.any()):
            failures.append(f"{name}: {int(lost.sum())} finite elements inside a cone (a NaN was lost), first at {lost.nonzero()[0].tolist()}")
        stray = bad & ~cone
        far = stray & ~mine
        if bool(far.any()):
            failures.append(f"{name}: {int(far.sum())} non-finite elements outside every plant's own rows / tile, first at {far.nonzero()[0].tolist()}")
        near = stray & mine & ~table
        if bool(near.any()):
            at = near.nonzero()
            failures.append(f"{name}: {int(near.sum())} non-finite elements outside the cone (own row / tile, no table entry), "
                            f"first at {at[0].tolist()}, last at {at[-1].tolist()}")
        if bool((stray & table).any()):
            deviations[name] = int((stray & table).sum())
        ok = ~(cone | bad)
        err = torch.where(ok, (torch.where(ok, g, 0.0) - ref[name].to(dev)).abs() / (R.U * S[name].to(dev) + 1e-300), 0.0)
        worst = float(err.max()) if err.numel() else 0.0
        if not worst <= 1.0:
            failures.append(f"{name}: outside the cones err / (U S) = {worst:.3g}")
    return failures, deviations


# ---------------------------------------------------------------------------------------------------------------------
# plants of a launch

def positions(L, tiles=(16, 160, 640), segment_starts=()):
    """the memory positions the tests plant at: the first four, the last, the first of the second 16- / 160- / 640-tile
    where the row has one, the first position of every sequence segment given"""
    ts = [0, 1, 2, 3, L - 1] + [t for t in tiles if t < L] + [t for t in segment_starts if 0 < t < L]
    return sorted(set(t for t in ts if 0 <= t < L))


def launches(operand, value, dims, rev_mask, u_gshift, dout_gshift, ts):
    """lists of plants, one list per launch, that between them put ``operand`` at every position of ``ts`` on a forward
    and on a reversed row (row operands: one element each way), each launch's cones pairwise disjoint: one plant per
    (batch image, group) on rows that differ -- per pair of groups where a shared u / dout row feeds two, per group for B
    and C (dA, dD and ddelta_bias of a row sum over the batch)"""
    batch, KD, L, N, G = dims
    rows = KD // G
    rev = lambda g: bool((rev_mask >> g) & 1)
    if operand in ROW_OPERANDS:
        gs = [next(g for g in range(G) if not rev(g))] + [g for g in range(G) if rev(g)][:1]
        plants = []
        for i, g in enumerate(gs):
            r = g * rows + (5 * i + 3) % rows
            plants.append(Plant(operand, (r, (2 * i + 1) % N) if operand == "A" else (r,), value))
        return [plants]
    sh = {"u": u_gshift, "dout": dout_gshift}.get(operand, 0)
    # cells: (batch image, "group" in the operand's own layout); which directions a cell serves
    if operand in ("u", "dout"):
        cells = [(b, gu) for b in range(batch) for gu in range(G >> sh)]
        dirs = lambda gu: {rev(g) for g in range(G) if (g >> sh) == gu}
    elif operand == "delta":
        cells = [(b, g) for b in range(batch) for g in range(G)]
        dirs = lambda g: {rev(g)}
    else:                                                     # B, C reach ddelta_bias of every row of their group, which
        cells = [(g % batch, g) for g in range(G)]            # sums over the batch: one plant per group
        dirs = lambda g: {rev(g)}
    want = []                                                 # (position, direction) still to serve
    for t in ts:
        for d in sorted({d for _, g in cells for d in dirs(g)}):
            want.append((t, d))
    out = []
    while want:
        plants, free = [], list(cells)
        for t, d in list(want):
            if (t, d) not in want:
                continue
            cell = next((c for c in free if d in dirs(c[1])), None)
            if cell is None:
                continue
            free.remove(cell)
            for dd in dirs(cell[1]):                          # a shared row serves both directions at once
                if (t, dd) in want:
                    want.remove((t, dd))
            b, g = cell
            k = len(plants)
            row = g * rows + (7 * k + 2) % rows
            if operand in ("B", "C"):
                plants.append(Plant(operand, (b, g, (3 * k + 1) % N, t), value))
            else:
                plants.append(Plant(operand, (b, row, t), value))
        out.append(plants)
    return out

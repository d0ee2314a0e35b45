"""Seeded LP generators standing in for the BASELINE.json configs whose .mps files are not in the
image (no network): configs[1] "Netlib 25fv47" and configs[4] "pds-20 or equivalent".

Test infrastructure.  Pure numpy/scipy (PCG64 streams are stable across numpy versions); nothing
from the reference.  Both generators build LPs that are primal AND dual feasible by construction
(a primal point inside all bounds; c = A'y* + z* with multiplier signs that match the row / bound
types), so an optimum exists and HiGHS (scipy.optimize.linprog) gives an independent optimal value.

  staircase_lp      "25fv47-class": ~820 rows x ~1570 columns, ~10 000 nonzeros, staircase
                    (multi-period) structure, mixed E / L / G / range rows, lower-bounded, boxed and
                    free columns, coefficient magnitudes over several decades.  (25fv47 itself:
                    821 rows, 1571 columns, 10 400 nonzeros.)
  multicommodity_lp "PDS-class" (patient distribution system = multicommodity flow with joint arc
                    capacities): K commodities on a random layered digraph; per commodity one flow
                    conservation row per node (equalities), joint capacity rows on a subset of the
                    arcs (inequalities), per-commodity arc bounds on some arcs.  At the default size
                    m ~ 3.4e4 rows like pds-20 (33 874 rows, 105 728 columns, 230 200 nonzeros).
  write_free_mps    free-format MPS writer (what the reference reads through QPSReader,
                    /root/reference/src/Interfaces/tulip_julia_api.jl:18-39), so that both backends
                    are fed "the same .mps input".
"""
import numpy as np
import scipy.sparse as sp

from ipm_harness import LP

INF = float("inf")


def _dual_feasible_cost(A, lcon, ucon, lvar, uvar, rng):
    """c = A'y + z with y_i free on E rows, <= 0 on L rows, >= 0 on G rows, 0 on range rows;
    z_j >= 0 for lower-bounded, <= 0 for upper-bounded only, any sign for boxed, 0 for free columns."""
    m, n = A.shape
    y = rng.standard_normal(m)
    only_u = np.isinf(lcon) & np.isfinite(ucon)
    only_l = np.isfinite(lcon) & np.isinf(ucon)
    rng_row = np.isfinite(lcon) & np.isfinite(ucon) & (lcon < ucon)
    y[only_u] = -np.abs(y[only_u]); y[only_l] = np.abs(y[only_l]); y[rng_row] = 0.0
    z = rng.uniform(0.1, 1.0, n)
    fin_l, fin_u = np.isfinite(lvar), np.isfinite(uvar)
    z[~fin_l & fin_u] *= -1.0
    boxed = fin_l & fin_u
    z[boxed] *= rng.choice([-1.0, 1.0], size=int(boxed.sum()))
    z[~fin_l & ~fin_u] = 0.0
    return A.T @ y + z


def staircase_lp(seed=25047, periods=12, rows_per=68, cols_per=131, name="STAIR25"):
    """Netlib-25fv47-class staircase LP (see the module docstring)."""
    rng = np.random.default_rng(seed)
    T = periods
    m, n = T * rows_per + 5, T * cols_per
    ri, ci, vv = [], [], []
    for t in range(T):
        r0, c0 = t * rows_per, t * cols_per
        for j in range(cols_per):
            k = int(rng.integers(3, 8))                            # within-period entries
            rr = rng.choice(rows_per, size=k, replace=False)
            ri += list(r0 + rr); ci += [c0 + j] * k
            vv += list(rng.standard_normal(k) * 10.0 ** rng.integers(-2, 3, k))
            if t + 1 < T and rng.random() < 0.45:                  # carry-over into the next period
                k2 = int(rng.integers(1, 3))
                rr = rng.choice(rows_per, size=k2, replace=False)
                ri += list(r0 + rows_per + rr); ci += [c0 + j] * k2
                vv += list(rng.standard_normal(k2))
        # a few rows of the period are dense-ish budget rows
    for q in range(5):                                             # global rows over a column sample
        cols = rng.choice(n, size=60, replace=False)
        ri += [T * rows_per + q] * 60; ci += list(cols); vv += list(rng.uniform(0.5, 2.0, 60))
    A = sp.csc_matrix((vv, (ri, ci)), shape=(m, n)); A.sum_duplicates(); A.sort_indices()
    # every row needs an entry: add a unit entry on a random column to empty rows
    empty = np.nonzero(np.diff(A.tocsr().indptr) == 0)[0]
    if empty.size:
        A = (A + sp.csc_matrix((np.ones(empty.size), (empty, rng.integers(0, n, empty.size))), shape=(m, n))).tocsc()
        A.sort_indices()
    # column bounds: 80 % [0, inf), 14 % boxed [0, u], 4 % free, 2 % (-inf, u]
    kind = rng.choice(4, size=n, p=[0.80, 0.14, 0.04, 0.02])
    lvar = np.zeros(n); uvar = np.full(n, INF)
    uvar[kind == 1] = rng.uniform(1.0, 10.0, int((kind == 1).sum()))
    lvar[kind == 2] = -INF
    lvar[kind == 3] = -INF; uvar[kind == 3] = rng.uniform(0.0, 5.0, int((kind == 3).sum()))
    x0 = rng.uniform(0.2, 0.9, n)
    x0[kind == 1] *= uvar[kind == 1]
    x0[kind == 2] = rng.standard_normal(int((kind == 2).sum()))
    x0[kind == 3] = uvar[kind == 3] - rng.uniform(0.1, 1.0, int((kind == 3).sum()))
    act = A @ x0
    # row types: 55 % E, 25 % L, 15 % G, 5 % range
    rt = rng.choice(4, size=m, p=[0.55, 0.25, 0.15, 0.05])
    slack = rng.uniform(0.05, 1.0, m) * (1 + np.abs(act))
    lcon = act.copy(); ucon = act.copy()
    lcon[rt == 1] = -INF; ucon[rt == 1] = (act + slack)[rt == 1]
    ucon[rt == 2] = INF; lcon[rt == 2] = (act - slack)[rt == 2]
    lcon[rt == 3] = (act - slack)[rt == 3]; ucon[rt == 3] = (act + slack)[rt == 3]
    c = _dual_feasible_cost(A, lcon, ucon, lvar, uvar, rng)
    return LP(A, c, 0.0, lcon, ucon, lvar, uvar, True, name)


def multicommodity_lp(seed=2020, nodes=3080, arcs_per_node=3, K=10, cap_frac=0.33, bound_frac=0.2, name="PDSEQ20"):
    """PDS-class multicommodity flow LP (see the module docstring).  Default size: K*nodes = 30 800
    conservation rows + ~3 050 joint capacity rows = ~33 850 rows, K*arcs = 92 400 columns."""
    rng = np.random.default_rng(seed)
    E = nodes * arcs_per_node
    tail = np.repeat(np.arange(nodes), arcs_per_node)
    # layered digraph with mostly local arcs (like a transport network): head = tail + small offset
    off = rng.integers(1, 40, E)
    far = rng.random(E) < 0.05
    off[far] = rng.integers(1, nodes, int(far.sum()))
    head = (tail + off) % nodes
    n = K * E
    # node-arc incidence per commodity (flow out of tail: +1, into head: -1)
    Ninc = sp.csc_matrix((np.concatenate([np.ones(E), -np.ones(E)]),
                          (np.concatenate([tail, head]), np.concatenate([np.arange(E), np.arange(E)]))), shape=(nodes, E))
    cons = sp.block_diag([Ninc] * K, format="csc")
    capped = np.nonzero(rng.random(E) < cap_frac)[0]
    ncap = capped.size
    J = sp.csc_matrix((np.ones(ncap), (np.arange(ncap), capped)), shape=(ncap, E))
    A = sp.vstack([cons, sp.hstack([J] * K, format="csc")], format="csc")
    A.sort_indices()
    m = K * nodes + ncap
    # a feasible multicommodity flow: random nonnegative arc flows; supplies = their divergence
    x0 = rng.uniform(0.0, 2.0, n) * (rng.random(n) < 0.6)
    b_cons = cons @ x0
    joint = (sp.hstack([J] * K, format="csc") @ x0)
    lcon = np.concatenate([b_cons, np.full(ncap, -INF)])
    ucon = np.concatenate([b_cons, joint + rng.uniform(0.5, 3.0, ncap)])
    lvar = np.zeros(n); uvar = np.full(n, INF)
    bd = rng.random(n) < bound_frac
    uvar[bd] = x0[bd] + rng.uniform(0.5, 2.0, int(bd.sum()))
    cost = np.tile(rng.uniform(1.0, 10.0, E), K) * rng.uniform(0.8, 1.2, n)      # positive arc costs: bounded below
    return LP(A, cost, 0.0, lcon, ucon, lvar, uvar, True, name)


def bump_lp(seed=99, m=60, n=160, pairs=20, big=3.0e5):
    """An LP engineered so that the normal-equations Cholesky FAILS numerically late in the IPM run
    and the reference's retry loop (/root/reference/src/IPM/HSD/step.jl:35-51: regularisations x100,
    up to 3 times) has to fire: `pairs` free columns with entries `big` and `2*big` in two rows each.
    For a free column theta_inv = 0, so D_j = 1/regP_j grows to 1/sqrt(eps) = 6.7e7 and the two rows
    become numerically parallel in S = A D A' + Rd (rank-one term ~ 6e18 against O(1) remainders):
    the Schur complement of the second row is positive in exact arithmetic and rounding noise of
    size ~1e3 in fp64."""
    rng = np.random.default_rng(seed)
    A = sp.random(m, n, density=4.0 / m, random_state=seed, format="lil", data_rvs=rng.standard_normal)
    for i in range(m):
        A[i, rng.integers(0, n)] = 1.0
    free_cols = []
    for q in range(pairs):
        j = n + q
        free_cols.append(j)
    B = sp.lil_matrix((m, pairs))
    rows = rng.permutation(m)[: 2 * pairs].reshape(pairs, 2)
    for q in range(pairs):
        B[rows[q, 0], q] = big; B[rows[q, 1], q] = 2.0 * big
    A = sp.hstack([A.tocsc(), B.tocsc()], format="csc"); A.sort_indices()
    ntot = n + pairs
    lvar = np.zeros(ntot); uvar = np.full(ntot, INF)
    lvar[n:] = -INF
    x0 = np.concatenate([rng.uniform(0.5, 1.5, n), rng.standard_normal(pairs) * 1e-3])
    b = A @ x0
    c = _dual_feasible_cost(A, b, b, lvar, uvar, rng)
    return LP(A, c, 0.0, b, b, lvar, uvar, True, "BUMP")


def planted_tree(nodes, seed):
    """A constraint matrix whose K1 analysis (natural ordering, relax=False) has EXACTLY the elimination tree asked for: `nodes` is a
    postorder list of (ns, parent) -- parent = index of a later node, or -1 for a root (several roots: a forest).  Node q owns ns_q
    consecutive rows.  A = [one pair of dense columns per node | I]; the pair of node q covers

        its own rows, its parent's rows EXCEPT the parent's first, and whatever the parent's pair covers above the parent's rows.

    In A D A' + Rd a pair is a clique on the rows it covers, so the columns of node q all have the structure {own rows from the diagonal
    down} + cover(q) above: one supernode.  Its last column's structure without the diagonal is one row longer than the parent's first
    column could match (the skipped row), so the fundamental-supernode rule never merges a child into its parent, and two children of one
    parent keep the parent's first column from merging with either.  Hence front q has ns = ns_q pivot columns and
    f = ns_q + (ns_parent - 1) + (f_parent - ns_parent) = ns_q + f_parent - 1 rows (a root: f = ns), and nchild = its children in `nodes`.
    (A parent of ONE row leaves none of its rows for a child to cover: the child would hang under the grandparent.  Refused.)

    Returns (A csc of N x (2 len(nodes) + N), [(ns, f, nchild) per node, in the order of `nodes`]); the values are N(0, 1), the unit
    columns are the slacks."""
    rng = np.random.default_rng(seed)
    ns = np.array([q[0] for q in nodes], dtype=np.int64)
    parent = [int(q[1]) for q in nodes]
    assert all(p == -1 or q < p < len(nodes) for q, p in enumerate(parent)) and (ns >= 1).all(), "postorder: a parent comes after its children"
    first = np.concatenate([[0], np.cumsum(ns)])
    N = int(first[-1])
    cover_above = [None] * len(nodes)                      # rows of the ancestors that the node's pair covers
    for q in range(len(nodes) - 1, -1, -1):
        p = parent[q]
        cover_above[q] = np.zeros(0, dtype=np.int64) if p < 0 else np.concatenate([np.arange(first[p] + 1, first[p + 1]), cover_above[p]])
        assert p < 0 or ns[p] > 1, "a child covers none of a one-row parent's rows: it would hang under the grandparent, or be a root"
    ri, ci = [], []
    for q in range(len(nodes)):
        rows = np.concatenate([np.arange(first[q], first[q + 1]), cover_above[q]])
        for c in (2 * q, 2 * q + 1):
            ri.append(rows); ci.append(np.full(len(rows), c))
    ri, ci = np.concatenate(ri), np.concatenate(ci)
    dense = sp.csc_matrix((rng.standard_normal(len(ri)), (ri, ci)), shape=(N, 2 * len(nodes)))
    A = sp.hstack([dense, sp.identity(N, format="csc")], format="csc"); A.sort_indices()
    nchild = np.bincount([p for p in parent if p >= 0], minlength=len(nodes))
    shapes = [(int(ns[q]), int(ns[q] + len(cover_above[q])), int(nchild[q])) for q in range(len(nodes))]
    return A, shapes


def planted_tree_k2(nodes, seed, transposed=False):
    """A constraint matrix and a permutation of the K2 nodes (variable j = node j, constraint i = node n + i) whose K2 analysis
    (ordering="user", relax=False) has EXACTLY the fronts asked for, each with the SIGN PATTERN asked for: `nodes` is a postorder list of
    (pattern, parent), pattern a string over '+' (a constraint node, pivot sign +1) and '-' (a variable node, -1) -- the signs of the
    front's pivot columns in elimination order.  Every pattern starts with '+', holds a '-', and a parent holds two '+' at least.

    Node q owns the rows of its '+', the columns of its '-' and one HELPER column.  The helper and every own column have entries on
    T_q = q's rows + cover(q), cover(q) = the parent's rows except the parent's first, then cover(parent) (the skipped-row rule of
    planted_tree).  The order is, node by node: the helper, then q's nodes as the pattern lists them.  In the graph of K2 a column is
    adjacent to its rows only.  The helper is eliminated first and makes T_q a clique: a leaf front of one column, f = 1 + |T_q|, sign -.
    q's first row then sees the rest of T_q and all of q's columns, and after it all of these are one clique: one supernode, whatever the
    order of the further pivots.  The helper does not merge into it (its column is |own columns| >= 1 entries short), q's last column is one
    row longer than the parent's first could match (the skipped row), and the parent's columns see no child's column.  Hence front q has
    ns = len(pattern), f = ns + |cover(q)| (the rows below are the ancestors' '+' rows) and nchild = its children in `nodes` + 1.

    transposed: the same tree with rows and columns exchanged (the matrix is the transpose) -- every pattern starts with '-', the helper
    is a ROW (a front of sign +) and the rows below a front are its ancestors' '-' columns.

    Returns (A csc, perm of length m + n, [(ns, f, nchild)], [sign string]), the last two per front in elimination order: the helper
    of node q is front 2q, node q is front 2q + 1.  The values are N(0, 1)."""
    if transposed:
        swap = str.maketrans("+-", "-+")
        A, perm, shapes, signs = planted_tree_k2([(pat.translate(swap), p) for pat, p in nodes], seed)
        m0, n0 = A.shape                                       # old variable j -> constraint j = node m0 + j; old constraint i -> variable i
        perm = np.where(perm < n0, perm + m0, perm - n0)
        return A.T.tocsc(), perm, shapes, [s.translate(swap) for s in signs]
    rng = np.random.default_rng(seed)
    parent = [int(q[1]) for q in nodes]
    assert all(p == -1 or q < p < len(nodes) for q, p in enumerate(parent)), "postorder: a parent comes after its children"
    for q, (pat, _) in enumerate(nodes):
        assert pat[0] == "+" and "-" in pat and set(pat) <= {"+", "-"}, f"node {q}: a pattern starts with '+' and holds a '-'"
    rows, cols, helper, order = [], [], [], []               # order: ('c', column) | ('r', row) in elimination order
    m = n = 0
    for pat, _ in nodes:
        helper.append(n); order.append(("c", n)); n += 1
        r, c = [], []
        for ch in pat:
            if ch == "+":
                r.append(m); order.append(("r", m)); m += 1
            else:
                c.append(n); order.append(("c", n)); n += 1
        rows.append(np.array(r, dtype=np.int64)); cols.append(np.array(c, dtype=np.int64))
    cover = [None] * len(nodes)
    for q in range(len(nodes) - 1, -1, -1):
        p = parent[q]
        cover[q] = np.zeros(0, dtype=np.int64) if p < 0 else np.concatenate([rows[p][1:], cover[p]])
        assert p < 0 or len(rows[p]) > 1, "a child covers none of the rows of a parent with one '+': it would hang under the grandparent"
    ri, ci = [], []
    for q in range(len(nodes)):
        T = np.concatenate([rows[q], cover[q]])
        for c in [helper[q]] + cols[q].tolist():
            ri.append(T); ci.append(np.full(len(T), c))
    ri, ci = np.concatenate(ri), np.concatenate(ci)
    A = sp.csc_matrix((rng.standard_normal(len(ri)), (ri, ci)), shape=(m, n)); A.sort_indices()
    perm = np.array([i if kind == "c" else n + i for kind, i in order], dtype=np.int64)
    nchild = np.bincount([p for p in parent if p >= 0], minlength=len(nodes))
    shapes, signs = [], []
    for q, (pat, _) in enumerate(nodes):
        shapes += [(1, 1 + len(rows[q]) + len(cover[q]), 0), (len(pat), len(pat) + len(cover[q]), int(nchild[q]) + 1)]
        signs += ["-", pat]
    return A, perm, shapes, signs


def write_free_mps(lp, path):
    """Free-format MPS (row names R<i>, column names C<j>, objective row COST).  Values are written
    with repr() so that reading the file back reproduces the LP bit for bit."""
    A = lp.A.tocsc(); m, n = A.shape
    with open(path, "w") as fh:
        fh.write(f"NAME {lp.name or 'LP'}\n")
        if not lp.objsense_min:
            fh.write("OBJSENSE\n    MAX\n")
        fh.write("ROWS\n N COST\n")
        rtype = []
        for i in range(m):
            lb, ub = lp.lcon[i], lp.ucon[i]
            t = "E" if lb == ub else ("L" if np.isinf(lb) and np.isfinite(ub) else ("G" if np.isfinite(lb) and np.isinf(ub) else "R"))
            if t == "R" and np.isinf(lb) and np.isinf(ub):
                raise ValueError("free rows are not written")
            rtype.append(t)
            fh.write(f" {'L' if t == 'R' else t} R{i}\n")
        fh.write("COLUMNS\n")
        for j in range(n):
            if lp.obj[j] != 0.0:
                fh.write(f" C{j} COST {float(lp.obj[j])!r}\n")
            for p in range(A.indptr[j], A.indptr[j + 1]):
                fh.write(f" C{j} R{A.indices[p]} {float(A.data[p])!r}\n")
            if lp.obj[j] == 0.0 and A.indptr[j] == A.indptr[j + 1]:
                fh.write(f" C{j} COST 0.0\n")
        fh.write("RHS\n")
        if lp.obj0 != 0.0:
            fh.write(f" RHS COST {float(-lp.obj0)!r}\n")
        for i in range(m):
            b = lp.ucon[i] if rtype[i] in ("L", "R", "E") else lp.lcon[i]
            if b != 0.0:
                fh.write(f" RHS R{i} {float(b)!r}\n")
        if "R" in rtype:
            fh.write("RANGES\n")
            for i in range(m):
                if rtype[i] == "R":
                    fh.write(f" RNG R{i} {float(lp.ucon[i] - lp.lcon[i])!r}\n")
        fh.write("BOUNDS\n")
        for j in range(n):
            lo, up = lp.lvar[j], lp.uvar[j]
            if lo == 0.0 and np.isinf(up):
                continue
            if np.isinf(lo) and np.isinf(up):
                fh.write(f" FR BND C{j}\n")
                continue
            if np.isinf(lo):
                fh.write(f" MI BND C{j}\n")
            elif lo != 0.0:
                fh.write(f" LO BND C{j} {float(lo)!r}\n")
            if np.isfinite(up):
                fh.write(f" UP BND C{j} {float(up)!r}\n")
        fh.write("ENDATA\n")

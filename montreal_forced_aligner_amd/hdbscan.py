"""HDBSCAN's cluster tree on the host: everything after the minimum spanning tree of the mutual-reachability graph, which is
O(N log N) work on N − 1 edges (the tree itself comes from the device: ``stats.mreach_mst``).

Restated from the papers — Campello, Moulavi, Sander, "Density-based clustering based on hierarchical density estimates" (2013):
the single-linkage hierarchy of the mutual-reachability tree, the condensed tree for ``min_cluster_size``, the stabilities
Σ (λ_point − λ_birth) and the excess-of-mass selection; McInnes, Healy, "Accelerated hierarchical density based clustering"
(2017): the condensed tree as a table of (parent, child, λ, size); Malzer, Baum, "A hybrid approach to hierarchical density-based
cluster selection" (2020): ``cluster_selection_epsilon`` — and held to ``sklearn.cluster.HDBSCAN`` as a black box
(tests/test_hdbscan_cpu.py).  λ = 1 / distance, +inf where the distance is not positive, which is scikit-learn's rule.  Clusters
are numbered by their smallest member; noise is −1.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

NOISE = -1


def single_linkage(n: int, lo, hi, dist) -> Tuple[List[int], List[int], List[float], List[int]]:
    """The hierarchy of a spanning tree whose ``n − 1`` edges come sorted by ascending distance: merge e makes node n + e of
    (left[e], right[e]) at value[e]; size[node] for every node (a point: 1)."""
    lo, hi, dist = [int(a) for a in lo], [int(b) for b in hi], [float(d) for d in dist]
    if len(lo) != max(n - 1, 0):
        raise ValueError(f"{len(lo)} edges for {n} points: a spanning tree has n - 1")
    parent = list(range(2 * n - 1)) if n > 0 else []
    size = [1] * n + [0] * max(n - 1, 0)
    left, right = [0] * len(lo), [0] * len(lo)
    for e in range(len(lo)):
        a, b = lo[e], hi[e]
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        if a == b:
            raise ValueError("the edges close a cycle: not a spanning tree")
        node = n + e
        left[e], right[e] = a, b
        parent[a] = parent[b] = node
        size[node] = size[a] + size[b]
    return left, right, dist, size


def condense_tree(n: int, linkage, min_cluster_size: int) -> Dict[str, np.ndarray]:
    """The condensed tree as rows (parent, child, lam, size): walking down from the root (cluster n), a split whose two sides both
    hold ``min_cluster_size`` points makes two new clusters; a side below it falls out of the parent point by point at the split's
    λ, and the other side stays the parent."""
    left, right, value, size = linkage
    rows_p: List[int] = []
    rows_c: List[int] = []
    rows_l: List[float] = []
    rows_s: List[int] = []
    if n < 2:
        return dict(parent=np.zeros(0, np.int64), child=np.zeros(0, np.int64), lam=np.zeros(0), size=np.zeros(0, np.int64))
    mcs = int(min_cluster_size)
    next_label = n + 1
    todo = [(2 * n - 2, n)]                      # (hierarchy node, the cluster it is)
    at = 0
    while at < len(todo):                         # breadth first: clusters are numbered level by level
        node, label = todo[at]
        at += 1
        e = node - n
        d = value[e]
        lam = 1.0 / d if d > 0.0 else float("inf")
        l, r = left[e], right[e]
        big_l, big_r = size[l] >= mcs, size[r] >= mcs
        for side, big, other_big in ((l, big_l, big_r), (r, big_r, big_l)):
            if big and other_big:
                rows_p.append(label); rows_c.append(next_label); rows_l.append(lam); rows_s.append(size[side])
                if side >= n:
                    todo.append((side, next_label))
                else:                              # min_cluster_size 1: a point as a cluster of its own
                    rows_p.append(next_label); rows_c.append(side); rows_l.append(lam); rows_s.append(1)
                next_label += 1
            elif big:
                if side >= n:
                    todo.append((side, label))
                else:
                    rows_p.append(label); rows_c.append(side); rows_l.append(lam); rows_s.append(1)
            else:
                stack = [side]                     # every point below falls out of the cluster here
                while stack:
                    x = stack.pop()
                    if x < n:
                        rows_p.append(label); rows_c.append(x); rows_l.append(lam); rows_s.append(1)
                    else:
                        stack.append(right[x - n]); stack.append(left[x - n])
    return dict(parent=np.asarray(rows_p, np.int64), child=np.asarray(rows_c, np.int64), lam=np.asarray(rows_l, np.float64),
                size=np.asarray(rows_s, np.int64))


def stabilities(n: int, tree) -> Dict[int, float]:
    """Every cluster's stability Σ over its rows of (λ_row − λ_birth) · size; the root is born at λ = 0."""
    parent, child, lam, size = tree["parent"], tree["child"], tree["lam"], tree["size"]
    birth = {n: 0.0}
    for c, l in zip(child.tolist(), lam.tolist()):
        if c >= n:
            birth[c] = l
    out: Dict[int, float] = {}
    with np.errstate(invalid="ignore"):
        for p, l, s in zip(parent.tolist(), lam.tolist(), size.tolist()):
            out[p] = out.get(p, 0.0) + (np.float64(l) - birth[p]) * s
    return {k: float(v) for k, v in out.items()}


def _cluster_rows(n: int, tree):
    m = tree["child"] >= n
    return tree["parent"][m], tree["child"][m], tree["lam"][m], tree["size"][m]


def select_clusters(n: int, tree, stability: Dict[int, float], cluster_selection_epsilon: float = 0.0) -> List[int]:
    """Excess of mass with the root excluded: from the leaves up, a cluster stays selected unless its children's total stability
    is larger, in which case it takes that total; then, for ε > 0, a selected cluster born at a distance below ε is replaced by its
    nearest ancestor born at a distance above ε (Malzer and Baum), the root excepted."""
    cp, cc, cl, _ = _cluster_rows(n, tree)
    children: Dict[int, List[int]] = {}
    parent_of: Dict[int, int] = {}
    birth_lam: Dict[int, float] = {}
    for p, c, l in zip(cp.tolist(), cc.tolist(), cl.tolist()):
        children.setdefault(p, []).append(c)
        parent_of[c] = p
        birth_lam[c] = l
    stab = dict(stability)
    nodes = sorted((k for k in stab if k != n), reverse=True)
    is_cluster = {k: True for k in nodes}

    def below(node):
        out, stack = [], list(children.get(node, []))
        while stack:
            x = stack.pop()
            out.append(x)
            stack.extend(children.get(x, []))
        return out
    for node in nodes:                             # descending numbers: a child has a larger number than its parent
        sub = sum(stab[c] for c in children.get(node, []))
        if sub > stab[node]:
            is_cluster[node] = False
            stab[node] = sub
        else:
            for x in below(node):
                is_cluster[x] = False
    selected = sorted(k for k, v in is_cluster.items() if v)
    eps = float(cluster_selection_epsilon)
    if eps != 0.0 and cc.shape[0] > 0:
        out, processed = [], set()
        for leaf in selected:
            with np.errstate(divide="ignore"):
                d = float(np.float64(1.0) / np.float64(birth_lam[leaf]))
            if d >= eps:
                out.append(leaf)
                continue
            if leaf in processed:
                continue
            node = leaf
            while True:
                p = parent_of[node]
                if p == n:                         # the root is no cluster: the node nearest to it
                    break
                node = p
                with np.errstate(divide="ignore"):
                    if float(np.float64(1.0) / np.float64(birth_lam[node])) > eps:
                        break
            out.append(node)
            processed.update(below(node))
        selected = sorted(set(out))
    return selected


def labels_from_clusters(n: int, tree, clusters) -> np.ndarray:
    """A point's label: the selected cluster it falls out of, or out of a descendant of; −1 otherwise.  Numbered by smallest member."""
    clusters = set(int(c) for c in clusters)
    owner: Dict[int, int] = {}                     # cluster → the selected cluster that holds it (or the root n)
    cp, cc, _, _ = _cluster_rows(n, tree)
    owner[n] = n
    for p, c in zip(cp.tolist(), cc.tolist()):     # rows come parents first
        owner[c] = c if c in clusters else owner[p]
    raw = np.full(n, n, np.int64)
    pts = tree["child"] < n
    for p, c in zip(tree["parent"][pts].tolist(), tree["child"][pts].tolist()):
        raw[c] = owner[p]
    labels = np.full(n, NOISE, np.int64)
    number: Dict[int, int] = {}
    for i in range(n):
        c = int(raw[i])
        if c == n:
            continue
        if c not in number:
            number[c] = len(number)
        labels[i] = number[c]
    return labels


def cluster_tree_labels(n: int, lo, hi, dist, min_cluster_size: int, cluster_selection_epsilon: float = 0.0) -> np.ndarray:
    """The labels of ``n`` points from the spanning tree's edges, sorted by ascending distance."""
    if int(min_cluster_size) < 2:
        raise ValueError(f"min_cluster_size {min_cluster_size}: 2 or more")
    if n < 2:
        return np.full(n, NOISE, np.int64)
    tree = condense_tree(n, single_linkage(n, lo, hi, dist), min_cluster_size)
    return labels_from_clusters(n, tree, select_clusters(n, tree, stabilities(n, tree), cluster_selection_epsilon))


__all__ = ["NOISE", "cluster_tree_labels", "condense_tree", "labels_from_clusters", "select_clusters", "single_linkage", "stabilities"]

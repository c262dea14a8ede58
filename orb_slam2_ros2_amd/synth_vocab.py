"""Deterministic vocabulary trees for the bag-of-words path, and a writer for the ORB-SLAM2 text format (include/orbfe.h).

A vocabulary is a dict: k, L and, in node-id order (the root is node 0), parent (int32, -1 for the root), is_leaf (uint8), desc
([n][32] uint8, zeros for the root), weight (float64) and word_id (int32, -1 for inner nodes; leaves numbered in node-id order).  Children
of a node are the nodes naming it as parent, in node-id order.

  trained(seed)          hierarchical k-majority over patch descriptors of synth frames, IDF weights ln(N / n_i) over the training
                         frames (a word seen in every frame weighs 0, a word no frame reaches keeps weight 0)
  edge(seed, k, L)       identical sibling descriptors (exact ties), single-child chains, leaves at every level 1..L, zero-weight leaves;
                         for k > 16 the root has exactly k children; from child 16 on, copies of children below 16 and one
                         descriptor of its own
  full(seed, k, L)       the complete k-ary tree of depth L with random descriptors and weights (k = 10, L = 6: 1 111 111 nodes)
  reorder_dfs(voc)       the same tree listed depth-first (every parent still before its children, not breadth-first)
  write_txt(path, voc)   the text file orbfe_vocab_load_txt reads
"""
from __future__ import annotations

import math

import numpy as np

from . import synth

_POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def hamming(a, b):
    """Hamming-256 distances of descriptor arrays that broadcast against each other ([..., 32] uint8)"""
    return _POP8[np.bitwise_xor(a, b)].sum(axis=-1, dtype=np.int32)


def patch_descriptors(img, n, seed):
    """n BRIEF-like 256-bit descriptors of an image: a hashed pattern of 256 pixel pairs inside a 31 x 31 patch, at n hashed positions"""
    h, w = img.shape
    idx = np.arange(n, dtype=np.uint64)
    xs = 16 + (synth.hash_u64(seed, 1, idx) % np.uint64(w - 32)).astype(np.int64)
    ys = 16 + (synth.hash_u64(seed, 2, idx) % np.uint64(h - 32)).astype(np.int64)
    pat = (synth.hash_u64(7, 3, np.arange(1024, dtype=np.uint64)) % np.uint64(31)).astype(np.int64).reshape(256, 4) - 15
    a = img[ys[:, None] + pat[None, :, 1], xs[:, None] + pat[None, :, 0]].astype(np.int16)
    b = img[ys[:, None] + pat[None, :, 3], xs[:, None] + pat[None, :, 2]].astype(np.int16)
    return np.packbits((a < b).astype(np.uint8), axis=1, bitorder="little")


def _majority(D):
    bits = np.unpackbits(D, axis=1, bitorder="little")
    return np.packbits((2 * bits.sum(axis=0) > len(D)).astype(np.uint8), bitorder="little")


def _finish(k, L, parent, is_leaf, desc, weight):
    parent = np.asarray(parent, np.int32)
    is_leaf = np.asarray(is_leaf, np.uint8)
    word_id = np.full(len(parent), -1, np.int32)
    word_id[is_leaf == 1] = np.arange(int(is_leaf.sum()), dtype=np.int32)
    return dict(k=int(k), L=int(L), parent=parent, is_leaf=is_leaf, desc=np.asarray(desc, np.uint8).reshape(-1, 32),
                weight=np.asarray(weight, np.float64), word_id=word_id)


def children(voc):
    """children lists in node-id (= file) order"""
    ch = [[] for _ in range(len(voc["parent"]))]
    for i, p in enumerate(voc["parent"][1:].tolist(), start=1):
        ch[p].append(i)
    return ch


def descend_leaves(voc, D):
    """leaf node of every descriptor of D under rule 1 (first minimum of the distances to the children in file order)"""
    ch = children(voc)
    kmax = max(1, max(len(c) for c in ch))
    tab = np.full((len(ch), kmax), -1, np.int64)
    for i, c in enumerate(ch):
        tab[i, :len(c)] = c
    cur = np.zeros(len(D), np.int64)
    for _ in range(voc["L"]):
        inner = voc["is_leaf"][cur] == 0
        if not inner.any():
            break
        C = tab[cur[inner]]
        d = hamming(D[inner][:, None, :], voc["desc"][np.maximum(C, 0)])
        d[C < 0] = 1 << 20
        cur[inner] = C[np.arange(len(C)), np.argmin(d, axis=1)]
    return cur


def trained(seed=0, k=10, L=4, n_frames=8, per_frame=1500, iters=3):
    """hierarchical k-majority over patch descriptors of n_frames synth frames (the four content classes in turn), IDF weights"""
    frames = []
    for f in range(n_frames):
        img, _ = synth.stereo_pair_content(f + 10 * seed, synth.CONTENT_CLASSES[f % len(synth.CONTENT_CLASSES)])
        frames.append(patch_descriptors(img, per_frame, seed * 1000 + f))
    D = np.concatenate(frames)
    rng = np.random.default_rng(seed)
    parent, is_leaf, desc, weight = [-1], [0], [np.zeros(32, np.uint8)], [0.0]
    queue = [(0, np.arange(len(D)), 0)]  # breadth first: node ids in DBoW's order
    while queue:
        nxt = []
        for node, members, depth in queue:
            X = D[members]
            m = min(k, len(np.unique(X, axis=0)))
            centers = X[rng.choice(len(X), size=m, replace=False)]
            for _ in range(iters):
                a = np.argmin(hamming(X[:, None, :], centers[None, :, :]), axis=1)
                centers = np.stack([_majority(X[a == c]) if (a == c).any() else centers[c] for c in range(m)])
            a = np.argmin(hamming(X[:, None, :], centers[None, :, :]), axis=1)
            for c in range(m):
                sel = members[a == c]
                if len(sel) == 0:
                    continue
                cid = len(parent)
                leaf = depth + 1 == L or len(sel) <= k
                parent.append(node), is_leaf.append(int(leaf)), desc.append(centers[c]), weight.append(0.0)
                if not leaf:
                    nxt.append((cid, sel, depth + 1))
        queue = nxt
    voc = _finish(k, L, parent, is_leaf, desc, weight)
    # IDF over the training frames (DBoW2 setNodeWeights): ln(N / n_i) for words some frame reaches, 0 for the rest
    seen = np.zeros(len(voc["parent"]), np.int64)
    for fd in frames:
        seen[np.unique(descend_leaves(voc, fd))] += 1
    for i in np.nonzero(seen)[0]:
        voc["weight"][i] = math.log(n_frames / int(seen[i]))
    return voc


def edge(seed=0, k=4, L=5, max_nodes=4000):
    """a random tree with every corner of the rules: identical sibling descriptors, single-child chains, leaves at every level 1..L,
    zero-weight leaves"""
    rng = np.random.default_rng(seed)
    parent, is_leaf, desc, weight = [-1], [0], [np.zeros(32, np.uint8)], [0.0]
    level = [(0, True)]  # (node, on the spine: kept inner down to L - 1)
    for depth in range(1, L + 1):
        nxt = []
        for node, spine in level:
            nc = 1 if (rng.random() < 0.25 and not spine) else int(rng.integers(2 if spine and k >= 2 else 1, k + 1))
            if spine and depth < L:
                nc = max(nc, min(2, k))
            if spine and depth == 1 and k > 16:
                nc = k   # children 16 .. k - 1 exist: the kernel's lanes take child j and j + 16
            kids = []
            for c in range(nc):
                if kids and rng.random() < 0.3:
                    d = desc[kids[int(rng.integers(len(kids)))]].copy()   # an exact copy of an earlier sibling: distance ties
                else:
                    d = rng.integers(0, 256, 32, dtype=np.uint8)
                if spine and depth < L and c == 0:
                    leaf, on_spine = False, True
                elif spine and c == nc - 1:
                    leaf, on_spine = True, False                         # a leaf at every level
                else:
                    leaf, on_spine = depth == L or len(parent) > max_nodes or rng.random() < 0.4, False
                w = 0.0 if rng.random() < 0.15 else float(rng.uniform(0.05, 3.0))
                if spine and depth == 1 and k > 16 and c >= 16:
                    # children from 16 on: exact ties with children below 16, in the same lane (16 / 0) and in other lanes (17 / 7, 19 / 12),
                    # and one of a descriptor of its own that only that child can win (18), with a weight that counts
                    if c % 4 == 2:
                        d, w = rng.integers(0, 256, 32, dtype=np.uint8), float(rng.uniform(0.05, 3.0))
                    else:
                        d = desc[kids[(0, 7, 0, 12)[c % 4]]].copy()
                cid = len(parent)
                parent.append(node), is_leaf.append(int(leaf)), desc.append(d), weight.append(w if leaf else 0.0)
                kids.append(cid)
                if not leaf:
                    nxt.append((cid, on_spine))
        level = nxt
    return _finish(k, L, parent, is_leaf, desc, weight)


def full(seed=0, k=10, L=6):
    """the complete k-ary tree of depth L, breadth first, random descriptors, random leaf weights (a tenth of them 0)"""
    sizes = [k ** d for d in range(L + 1)]
    n = sum(sizes)
    rng = np.random.default_rng(seed)
    parent = np.empty(n, np.int32)
    parent[0] = -1
    start = 1
    for d in range(1, L + 1):
        prev = start - sizes[d - 1]
        parent[start:start + sizes[d]] = prev + np.arange(sizes[d]) // k
        start += sizes[d]
    is_leaf = np.zeros(n, np.uint8)
    is_leaf[n - sizes[L]:] = 1
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    desc[0] = 0
    weight = np.zeros(n)
    w = rng.uniform(0.01, 8.0, sizes[L])
    w[rng.random(sizes[L]) < 0.1] = 0.0
    weight[n - sizes[L]:] = w
    return _finish(k, L, parent, is_leaf, desc, weight)


def reorder_dfs(voc):
    """the same tree renumbered depth-first (pre-order, siblings in their order): parents before children, not breadth-first"""
    ch = children(voc)
    order, stack = [], [0]
    while stack:
        i = stack.pop()
        order.append(i)
        stack.extend(reversed(ch[i]))
    order = np.asarray(order, np.int64)
    new_of = np.empty(len(order), np.int64)
    new_of[order] = np.arange(len(order))
    par = voc["parent"][order].astype(np.int64)
    par[1:] = new_of[par[1:]]
    return _finish(voc["k"], voc["L"], par, voc["is_leaf"][order], voc["desc"][order], voc["weight"][order])


_BYTE_TXT = np.frombuffer(b"".join(b"%4d" % i for i in range(256)), np.uint8).reshape(256, 4)


def write_txt(path, voc):
    """the ORB-SLAM2 text format: `k L 0 0`, then one line `parent is_leaf b0 .. b31 weight` per node after the root (fixed-width
    columns, weights as shortest round-trip decimals)"""
    n = len(voc["parent"]) - 1
    if n <= 0:
        with open(path, "w") as f:
            f.write(f"{voc['k']} {voc['L']} 0 0\n")
        return
    par = np.char.rjust(voc["parent"][1:].astype(str), 8).astype("S8").view(np.uint8).reshape(n, 8)
    leaf = (voc["is_leaf"][1:].astype(np.uint8) + ord("0")).reshape(n, 1)
    sp = np.full((n, 1), ord(" "), np.uint8)
    body = _BYTE_TXT[voc["desc"][1:]].reshape(n, 128)
    uniq, inv = np.unique(voc["weight"][1:], return_inverse=True)
    txt = [repr(float(v)).encode() for v in uniq]
    width = max(len(t) for t in txt)
    wt = np.frombuffer(b"".join(t.rjust(width) for t in txt), np.uint8).reshape(len(uniq), width)[inv.reshape(-1)]
    nl = np.full((n, 1), ord("\n"), np.uint8)
    rows = np.concatenate([par, sp, leaf, body, sp, wt, nl], axis=1)
    with open(path, "wb") as f:
        f.write(f"{voc['k']} {voc['L']} 0 0\n".encode())
        f.write(rows.tobytes())

"""The checker of the bag-of-words path: DBoW2 / DBoW3 TemplatedVocabulary::transform (binary features, L1 scoring, TF-IDF) and
L1Scoring::score restated in plain Python / numpy, over the arrays orb_slam2_ros2_amd.synth_vocab generated -- never over the library's
own parse, so a parser bug cannot hide.  The rules are those of the header comment of orb_slam2_ros2_amd/csrc/k_bow.hip."""
import numpy as np

from orb_slam2_ros2_amd.synth_vocab import children, hamming


def _table(voc):
    ch = children(voc)
    kmax = max(1, max(len(c) for c in ch))
    tab = np.full((len(ch), kmax), -1, np.int64)
    for i, c in enumerate(ch):
        tab[i, :len(c)] = c
    return tab


def descend(voc, desc, levelsup, tab=None):
    """(leaf, node) of every descriptor: rule 1 (first minimum over the children in file order, stop at a leaf) and rule 2 (the node at
    level L - levelsup, the root if that is <= 0, the leaf itself if the leaf comes first)"""
    tab = _table(voc) if tab is None else tab
    D = np.asarray(desc, np.uint8).reshape(-1, 32)
    n = len(D)
    nid_level = voc["L"] - levelsup
    cur = np.zeros(n, np.int64)
    node = np.zeros(n, np.int64) if nid_level <= 0 else np.full(n, -1, np.int64)
    for level in range(1, voc["L"] + 1):
        inner = voc["is_leaf"][cur] == 0
        if not inner.any():
            break
        C = tab[cur[inner]]
        d = hamming(D[inner][:, None, :], voc["desc"][np.maximum(C, 0)])
        d[C < 0] = 1 << 20
        cur[inner] = C[np.arange(len(C)), np.argmin(d, axis=1)]   # np.argmin: the FIRST minimum
        if level == nid_level:
            node[inner] = cur[inner]
    node[node < 0] = cur[node < 0]
    return cur, node


def transform(voc, desc, levelsup, tab=None):
    """(words, values, nodes, offsets, features) exactly as the library returns them"""
    leaf, node = descend(voc, desc, levelsup, tab)
    bow, fv = {}, {}
    for f in range(len(leaf)):
        w = float(voc["weight"][leaf[f]])
        if not w > 0:                                   # rule 3
            continue
        wid = int(voc["word_id"][leaf[f]])
        bow[wid] = bow.get(wid, 0.0) + w                # rule 4: BowVector::addWeight, in feature order
        fv.setdefault(int(node[f]), []).append(f)       # rule 5: FeatureVector::addFeature, in feature order
    words = sorted(bow)
    norm = 0.0
    for wid in words:
        norm += abs(bow[wid])
    values = [bow[wid] / norm if norm > 0 else bow[wid] for wid in words]
    nodes = sorted(fv)
    offsets, feats = [0], []
    for nd in nodes:
        feats += fv[nd]
        offsets.append(len(feats))
    return (np.asarray(words, np.uint32), np.asarray(values, np.float64), np.asarray(nodes, np.uint32), np.asarray(offsets, np.int32),
            np.asarray(feats, np.uint32))


def score_l1(a: dict, b: dict) -> float:
    """L1Scoring::score: merge over the common words in ascending order, s += |v - w| - |v| - |w|, return -s / 2"""
    s = 0.0
    for wid in sorted(set(a) & set(b)):
        v, w = a[wid], b[wid]
        s += abs(v - w) - abs(v) - abs(w)
    return -s / 2.0


def assert_same(got, want, what=""):
    """bit-equality of two transform results (values compared as int64 views)"""
    names = ("words", "values", "nodes", "offsets", "features")
    for name, g, w in zip(names, got, want):
        assert g.shape == w.shape, f"{what} {name}: shape {g.shape} != {w.shape}"
        if name == "values":
            assert np.array_equal(g.view(np.int64), w.view(np.int64)), f"{what} values differ"
        else:
            assert np.array_equal(g.astype(np.int64), w.astype(np.int64)), f"{what} {name} differ"

"""The checker of the keyframe database: KeyFrameDB's queries (src/KeyFrameDB.cc) restated in plain Python over dicts and sets of ids.
A keyframe is a BowVector {word: value}; `bad` is the set of ids whose isBad() is true; `conn[id]` is a keyframe's ordered covisible list
(getOrderedConnectedKfs(10)).  The decisions of DESIGN 4.15: keyframes in ascending id order, Group::mfAccScore starts at 0."""
import numpy as np

from bow_restatement import score_l1


class Restatement:
    def __init__(self):
        self.kfs = {}     # id -> {word: value}
        self.bad = set()

    def add(self, kf_id, bow):
        self.kfs.setdefault(kf_id, dict(bow))   # a std::set: adding an id twice changes nothing

    def erase(self, kf_id):
        self.kfs.pop(kf_id, None)
        self.bad.discard(kf_id)

    def set_bad(self, kf_id, flag=True):
        (self.bad.add if flag else self.bad.discard)(kf_id)

    # getKfAndWordDB: +1 per shared word for every listed keyframe that is neither bad nor ignored
    def counts(self, q, ignore=()):
        ignore = set(ignore)
        out = {}
        for kf_id, bow in self.kfs.items():
            if kf_id in self.bad or kf_id in ignore:
                continue
            c = len(q.keys() & bow.keys())   # one +1 per query word the keyframe lists
            if c:
                out[kf_id] = c
        return out

    def query(self, q, ignore=(), min_score=None):
        """{id: (count, score)} of the survivors of minWordFilter and, with min_score, minScoreFilter"""
        cnt = min_word_filter(self.counts(q, ignore))
        out = {k: (c, score_l1(q, self.kfs[k])) for k, c in cnt.items()}
        if min_score is not None:
            out = {k: v for k, v in out.items() if not v[1] < min_score}
        return dict(sorted(out.items()))

    def min_score(self, q, connected):
        """minScoreFilter's floor: 0 without connected keyframes, else 1 lowered to the smallest score of a non-bad one"""
        if not connected:
            return 0.0
        m = 1.0
        for k in connected:
            if k in self.bad:
                continue
            s = score_l1(q, self.kfs[k])
            if s < m:
                m = s
        return m

    def reloc(self, q, conn):
        return group_filter(self.query(q), conn, self.bad)

    def loop(self, q, all_connected, connected15, conn):
        ignore = [k for k in all_connected if k not in self.bad]
        return group_filter(self.query(q, ignore, self.min_score(q, connected15)), conn, self.bad)


def min_word_filter(cnt):
    """float th1 = (float)maxWordNum * 0.8; drop count < th1 (the count converted to float)"""
    mx = max(cnt.values(), default=0)
    th1 = np.float32(float(np.float32(mx)) * 0.8)
    return {k: c for k, c in cnt.items() if not np.float32(c) < th1}


def group_filter(survivors, conn, bad=frozenset()):
    """groupFilter over {id: (count, score)} in ascending id order; conn[id] the ordered covisible ids.  Returns the sorted candidates."""
    groups = []
    best_acc = 0.0
    for k in sorted(survivors):
        best, best_score = k, survivors[k][1]
        acc = 0.0
        acc += best_score
        for c in conn.get(k, ()):
            if c in bad or c not in survivors:
                continue
            s = survivors[c][1]
            acc += s
            if s > best_score:
                best, best_score = c, s
        groups.append((acc, best))
        if acc > best_acc:
            best_acc = acc
    th2 = best_acc * 0.75
    return sorted({best for acc, best in groups if acc > th2})

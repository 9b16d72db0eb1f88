"""Sequential restatement of the loop-candidate semantics (include/dvslam_hip.h, "loop candidates"): a keyframe database with a direct
index, and the node-guided, ratio-tested, one-to-one match of a query frame against an entry.  Plain Python on top of tests/bow_ref.py
(transform, Database), one feature after another, written from the header's rule and independently of csrc/loop.hip.  Integers only.

match() also returns, per candidate, counters of the paths the rule took, so that a test can show its inputs reach every one:
  one_member   query features whose node holds exactly one entry feature (d2 = 256)
  ratio        query features rejected by the ratio inequality alone (their d1 passed max_distance)
  distance     query features rejected by max_distance
  lost         proposals that lost their entry feature to a smaller (d1, i)
  d1_eq_d2     query features whose two best distances are equal"""
import numpy as np

import bow_ref as br

INT32_MAX = 2 ** 31 - 1
COUNTERS = ("one_member", "ratio", "distance", "lost", "d1_eq_d2")


class LoopDatabase:
    def __init__(self, voc, di_levels=0):
        assert di_levels >= 0
        self.voc, self.di_levels = voc, di_levels
        self.inv = br.Database(voc)              # the inverted part: the BowVector does not depend on levelsup
        self.fvs, self.rows = [], []

    def size(self):
        return len(self.rows)

    def clear(self):
        self.inv.clear()
        self.fvs, self.rows = [], []

    def add(self, feats):
        feats = np.asarray(feats, np.uint8).reshape(-1, 32).copy()
        _, _, fv, _ = br.transform(self.voc, feats, self.di_levels)
        self.fvs.append(fv)
        self.rows.append(feats)
        return self.inv.add(feats)

    def query(self, feats, max_results=0, max_id=-1):
        return self.inv.query(feats, max_results, max_id)

    def retrieve_features(self, entry_id):
        return self.fvs[entry_id]

    def proposals(self, feats, entry_id, max_distance=50, ratio=(3, 4), counters=None):
        """{i: (j1, d1)} before the one-to-one step"""
        feats = np.asarray(feats, np.uint8).reshape(-1, 32)
        num, den = ratio
        _, _, qfv, _ = br.transform(self.voc, feats, self.di_levels)
        efv = dict(self.fvs[entry_id])
        rows = self.rows[entry_id]
        out = {}
        for node, q_idx in qfv:
            if node not in efv:
                continue
            e_idx = efv[node]
            for i in q_idx:
                d1, j1, d2 = None, None, 256
                for j in e_idx:                                   # ascending j
                    d = br.hamming(feats[i], rows[j])
                    if d1 is None:
                        d1, j1 = d, j
                    elif d < d1:                                  # strict: the lowest j keeps a tie
                        d2, d1, j1 = d1, d, j
                    elif d < d2:
                        d2 = d
                if counters is not None:
                    counters["one_member"] += len(e_idx) == 1
                    counters["d1_eq_d2"] += d1 == d2
                if d1 > max_distance:
                    if counters is not None:
                        counters["distance"] += 1
                    continue
                if d1 * den > d2 * num:
                    if counters is not None:
                        counters["ratio"] += 1
                    continue
                out[i] = (j1, d1)
        return out

    def match_one(self, feats, entry_id, max_distance=50, ratio=(3, 4)):
        """(train_idx[n], dist[n], n_matches, counters) against one entry"""
        n = len(np.asarray(feats, np.uint8).reshape(-1, 32))
        counters = dict.fromkeys(COUNTERS, 0)
        prop = self.proposals(feats, entry_id, max_distance, ratio, counters)
        best = {}
        for i in sorted(prop):
            j, d = prop[i]
            if j not in best or (d, i) < best[j]:
                best[j] = (d, i)
        train = np.full(n, -1, np.int32); dist = np.full(n, INT32_MAX, np.int32)
        for i, (j, d) in prop.items():
            if best[j] == (d, i):
                train[i], dist[i] = j, d
            else:
                counters["lost"] += 1
        return train, dist, int((train >= 0).sum()), counters

    def match(self, feats, entry_ids, max_distance=50, ratio=(3, 4)):
        """(train_idx[c, n], dist[c, n], n_matches[c], [counters per candidate]); an id out of range: -1 and nothing matched"""
        n = len(np.asarray(feats, np.uint8).reshape(-1, 32))
        c = len(entry_ids)
        train = np.full((c, n), -1, np.int32); dist = np.full((c, n), INT32_MAX, np.int32); nm = np.zeros(c, np.int32)
        counters = []
        for x, e in enumerate(entry_ids):
            if e < 0 or e >= self.size():
                nm[x] = -1
                counters.append(dict.fromkeys(COUNTERS, 0))
                continue
            train[x], dist[x], nm[x], cnt = self.match_one(feats, int(e), max_distance, ratio)
            counters.append(cnt)
        return train, dist, nm, counters

    def detect(self, feats, max_results=4, max_id=-1, max_distance=50, ratio=(3, 4)):
        res = self.query(feats, max_results, max_id)
        ids = [e for e, _ in res]
        train, dist, nm, _ = self.match(feats, ids, max_distance, ratio)
        return ids, [s for _, s in res], nm, train, dist


# ---------------------------------------------------------------- the standard scene of the tests

def standard_scene():
    """(voc, entries, query): four entries on make_vocabulary(8, 10, 3), entry 1 with its first 7 rows appended again; the query is entry
    1 seen again — 80 % of its rows kept, 0..13 bit flips each, 20 random rows and 6 duplicated rows added, shuffled (PCG64(5))"""
    voc = br.make_vocabulary(8, 10, 3)
    entries = [br.make_features(voc, 40 + s, 300) for s in range(4)]
    entries[1] = np.concatenate([entries[1], entries[1][:7]])
    rng = np.random.Generator(np.random.PCG64(5))
    src = entries[1]
    keep = np.sort(rng.choice(len(src), size=len(src) * 8 // 10, replace=False))
    q = src[keep].copy()
    for r in q:
        for b in rng.choice(256, size=int(rng.integers(0, 14)), replace=False):
            r[b >> 3] ^= np.uint8(1 << (b & 7))
    extra = rng.integers(0, 256, (20, 32), dtype=np.uint8)
    dup = q[rng.choice(len(q), size=6, replace=False)].copy()
    q = np.concatenate([q, extra, dup])
    q = q[rng.permutation(len(q))]
    return voc, entries, np.ascontiguousarray(q)


def one_node_vocabulary(seed=3, k=4, L=2):
    """no zero weights: with di_levels >= L every feature of every frame lies under node 0, one segment per entry"""
    return br.make_vocabulary(seed, k, L, zero_weights=False)


def random_rows(seed, n):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (n, 32), dtype=np.uint8)


def near_rows(seed, base, n, max_flips=40):
    """n rows, each a row of `base` with 0..max_flips bits flipped: distances spread around the defaults' thresholds"""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = base[rng.integers(0, len(base), n)].copy() if len(base) and n else np.zeros((n, 32), np.uint8)
    for r in out:
        for b in rng.choice(256, size=int(rng.integers(0, max_flips + 1)), replace=False):
            r[b >> 3] ^= np.uint8(1 << (b & 7))
    return out

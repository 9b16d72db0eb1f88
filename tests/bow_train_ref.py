"""Sequential restatement of vocabulary training (include/dvslam_hip.h, "vocabulary training"): DBoW2's TemplatedVocabulary::create,
HKmeansStep, initiateClustersKMpp, FORB::meanValue and setNodeWeights, written from the published algorithm as it reads — recursive and
depth-first, one node after another — independently of the level-wise kernels of csrc/bow_train.hip.  Every quantity is an integer
except the final math.log (glibc's log on both sides).  PARITY UNPINNED: DBoW2 itself is not available here.

Stated choices: the sampler (DBoW2 seeds its random source from the clock), an iteration cap per node, and an emptied cluster keeps its
previous centre.  Also the deterministic training sets of the tests (PCG64 seeds)."""
import math
import numpy as np

import bow_ref as br

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
REPORT_FIELDS = ("n_nodes", "n_words", "levels_run", "max_passes", "nodes_capped", "clusters_emptied", "nodes_short_seeded")


def splitmix64(x):
    x = (x + GOLDEN) & MASK
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def draw(key, j):
    return splitmix64((key + j * GOLDEN) & MASK)


def distances(F, centre):
    """Hamming distance of every row of F to one descriptor"""
    return br._POP[np.bitwise_xor(F, centre)].sum(axis=1).astype(np.int64)


def mean_value(rows):
    """FORB::meanValue: bit b is set iff at least N/2 + N%2 of the N >= 1 rows have it set"""
    n = len(rows)
    assert n >= 1
    ones = np.unpackbits(rows, axis=1).sum(axis=0)
    return np.packbits(ones >= n // 2 + n % 2)


def seed_kmpp(F, k, key):
    """initiateClustersKMpp with the stated sampler: positions of the centres within F, in the order drawn (fewer than k when the
    remaining features all coincide with a centre)"""
    n = len(F)
    picked = [draw(key, 0) % n]
    min_dist = distances(F, F[picked[0]])
    j = 1
    while len(picked) < k:
        S = int(min_dist.sum())
        if S == 0:
            break
        cut = 1 + draw(key, j) % S
        running, pos = 0, None
        for i in range(n):                                      # the first position whose inclusive prefix sum reaches cut
            running += int(min_dist[i])
            if running >= cut:
                pos = i
                break
        picked.append(pos)
        min_dist = np.minimum(min_dist, distances(F, F[pos]))
        j += 1
    return picked


def associate(F, centres):
    """index of the centre of smallest distance per row; strict <: the first centre wins ties"""
    best = distances(F, centres[0])
    who = np.zeros(len(F), np.int64)
    for c in range(1, len(centres)):
        d = distances(F, centres[c])
        closer = d < best
        best = np.where(closer, d, best)
        who = np.where(closer, c, who)
    return who


class _Trainer:
    def __init__(self, feats, k, L, seed, max_iterations):
        self.feats, self.k, self.L, self.max_iterations = feats, k, L, max_iterations
        self.parent, self.desc = [], []
        self.report = dict.fromkeys(REPORT_FIELDS, 0)
        self.step(0, splitmix64(seed & MASK), list(range(len(feats))), 1)

    def step(self, parent_id, key, members, level):
        """HKmeansStep: `members` are positions in the training set, in order"""
        if not members:
            return
        rep = self.report
        rep["levels_run"] = max(rep["levels_run"], level)
        F = self.feats[members]
        if len(members) <= self.k:
            centres = [F[i].copy() for i in range(len(members))]
            groups = [[i] for i in range(len(members))]
        else:
            centres = [F[p].copy() for p in seed_kmpp(F, self.k, key)]
            if len(centres) < self.k:
                rep["nodes_short_seeded"] += 1
            last, passes, groups = None, 0, None
            while True:
                if passes >= 1:
                    for c, g in enumerate(groups):
                        if g:
                            centres[c] = mean_value(F[g])        # an emptied cluster keeps its previous centre
                who = associate(F, centres)
                groups = [np.nonzero(who == c)[0].tolist() for c in range(len(centres))]
                passes += 1
                if passes >= 2 and (who == last).all():
                    break
                if passes >= self.max_iterations:
                    rep["nodes_capped"] += 1
                    break
                last = who
            rep["max_passes"] = max(rep["max_passes"], passes)
            rep["clusters_emptied"] += sum(1 for g in groups if not g)
        ids = []
        for c in centres:
            self.parent.append(parent_id); self.desc.append(c)
            ids.append(len(self.parent))
        if level < self.L:
            for c, g in enumerate(groups):
                if len(g) > 1:
                    self.step(ids[c], splitmix64(key ^ (c + 1)), [members[i] for i in g], level + 1)


def train(feats, k, L, seed=0, max_iterations=100):
    """the tree alone: (parent ids, descriptors, report) of all features in image order"""
    t = _Trainer(np.asarray(feats, np.uint8).reshape(-1, 32), k, L, seed, max_iterations)
    return t.parent, np.array(t.desc, np.uint8).reshape(-1, 32), dict(t.report)


def weigh(tree, images, k, L, weighting):
    """setNodeWeights on a trained tree.  Returns (bow_ref.Vocabulary, report dict)"""
    parent, desc, report = tree
    n = len(parent)
    has_child = [False] * (n + 1)
    for p in parent:
        has_child[p] = True
    leaf = [0 if has_child[j + 1] else 1 for j in range(n)]
    voc = br.Vocabulary(k, L, br.L1_NORM, weighting, parent, leaf, desc, np.zeros(n))
    weight = np.zeros(n, np.float64)
    if weighting in (br.TF, br.BINARY):
        weight[np.asarray(leaf, bool)] = 1.0
    elif n:                                                     # Ni = images with a feature on the word, by the ordinary descent
        word_node = [j for j in range(n) if leaf[j]]
        Ni = [0] * voc.n_words
        for im in images:
            for w in sorted({br.transform_feature(voc, f)[0] for f in im}):
                Ni[w] += 1
        for w, j in enumerate(word_node):
            if Ni[w] > 0:
                weight[j] = math.log(float(len(images)) / float(Ni[w]))
    voc = br.Vocabulary(k, L, br.L1_NORM, weighting, parent, leaf, desc, weight)
    report = dict(report)
    report["n_nodes"], report["n_words"] = voc.n_nodes, voc.n_words
    return voc, report


def create(images, k, L, weighting=br.TF_IDF, seed=0, max_iterations=100):
    """OrbVocabulary::create.  images: list of (n_i, 32) uint8 arrays.  Returns (bow_ref.Vocabulary, report dict)"""
    images = [np.asarray(im, np.uint8).reshape(-1, 32) for im in images]
    feats = np.concatenate(images) if images else np.zeros((0, 32), np.uint8)
    return weigh(train(feats, k, L, seed, max_iterations), images, k, L, weighting)


# ---------------------------------------------------------------- training sets

def uniform(seed, n):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def clustered(seed, n):
    """7 random centres; every feature is one of them with 0..19 distinct bits flipped"""
    rng = np.random.Generator(np.random.PCG64(seed))
    centres = rng.integers(0, 256, (7, 32), dtype=np.uint8)
    out = np.zeros((n, 32), np.uint8)
    for i in range(n):
        d = centres[int(rng.integers(0, 7))].copy()
        for b in rng.choice(256, size=int(rng.integers(0, 20)), replace=False):
            d[b >> 3] ^= np.uint8(1 << (b & 7))
        out[i] = d
    return out


def dups(seed, n):
    """features drawn from only 3 distinct descriptors"""
    rng = np.random.Generator(np.random.PCG64(seed))
    base = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    return base[rng.integers(0, 3, n)]


GENERATORS = {"uniform": uniform, "clustered": clustered, "dups": dups}


def split(feats, counts):
    """the rows as consecutive images of the given sizes"""
    assert sum(counts) == len(feats)
    out, at = [], 0
    for c in counts:
        out.append(feats[at:at + c]); at += c
    return out


def five_images(n):
    """5 unequal image sizes adding up to n, the third of them 0"""
    a, b, d = n // 2, n // 5, n // 7
    return [a, b, 0, d, n - a - b - d]

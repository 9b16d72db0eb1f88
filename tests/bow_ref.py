"""Sequential restatement of the DBoW2 semantics the place-recognition kernels implement (include/dvslam_hip.h, "place recognition"):
TemplatedVocabulary<FORB::TDescriptor, FORB> — text format, one feature -> word, a frame -> BowVector / FeatureVector — and
TemplatedDatabase — add, query with L1 scoring.  Plain Python floats (IEEE doubles), one operation after another in the order DBoW2's
loops run; written from the published algorithm, independently of csrc/bow.hip.  PARITY UNPINNED: DBoW2 itself is not available here.
Two stated deviations: the node id of a feature whose descent ends at a leaf above level L - levelsup is that leaf (DBoW2 leaves it
uninitialised), and query results are ordered by (raw, entry id) (DBoW2: an unstable sort on raw alone).

Also the deterministic synthetic vocabularies and frames of the tests (PCG64 seeds)."""
import numpy as np

L1_NORM = 0
TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


class Vocabulary:
    """node 0 is the root; arrays index nodes 1 .. n as rows 0 .. n - 1"""

    def __init__(self, k, L, scoring, weighting, parent, is_leaf, desc, weight):
        self.k, self.L, self.scoring, self.weighting = int(k), int(L), int(scoring), int(weighting)
        self.parent = np.asarray(parent, np.int32).reshape(-1)
        self.is_leaf = np.asarray(is_leaf, np.uint8).reshape(-1)
        self.desc = np.asarray(desc, np.uint8).reshape(-1, 32)
        self.weight = np.asarray(weight, np.float64).reshape(-1)
        n = len(self.parent)
        self.children = [[] for _ in range(n + 1)]
        self.word_id = [-1] * (n + 1)
        self.n_words = 0
        for j in range(n):
            nid = j + 1
            assert 0 <= self.parent[j] < nid
            self.children[self.parent[j]].append(nid)          # child order is file order
            if self.is_leaf[j]:
                self.word_id[nid] = self.n_words
                self.n_words += 1
        self.n_nodes = n

    def node_desc(self, nid):
        return self.desc[nid - 1]

    def node_weight(self, nid):
        return float(self.weight[nid - 1])


def write_text(voc, path):
    """the format OrbVocabulary::loadFromTextFile reads: 'k L s w', then 'parent is_leaf d0 .. d31 weight' per node"""
    with open(path, "w") as fh:
        fh.write(f"{voc.k} {voc.L} {voc.scoring} {voc.weighting}\n")
        for j in range(voc.n_nodes):
            fh.write(f"{int(voc.parent[j])} {int(voc.is_leaf[j])} " + " ".join(str(int(b)) for b in voc.desc[j]) + f" {float(voc.weight[j])!r}\n")


def parse_text(path):
    with open(path) as fh:
        k, L, s, w = (int(t) for t in fh.readline().split())
        parent, leaf, desc, weight = [], [], [], []
        for line in fh:
            t = line.split()
            if not t:
                continue
            assert len(t) == 35, line
            parent.append(int(t[0])); leaf.append(1 if int(t[1]) > 0 else 0)
            desc.append([int(b) for b in t[2:34]]); weight.append(float(t[34]))
    return Vocabulary(k, L, s, w, parent, leaf, np.array(desc, np.uint8).reshape(-1, 32), weight)


def hamming(a, b):
    return int(_POP[np.bitwise_xor(a, b)].sum())


def transform_feature(voc, feat, levelsup=0, ties=None):
    """(word id, node id, weight) of one feature.  ties: a list that receives 1 per level at which the best distance was shared"""
    nid_level = voc.L - levelsup
    nid = 0 if nid_level <= 0 else None
    final, level = 0, 0
    while True:
        level += 1
        kids = voc.children[final]
        dists = _POP[np.bitwise_xor(voc.desc[np.asarray(kids) - 1], feat)].sum(axis=1).tolist()    # Hamming distance to every child
        final, best = kids[0], dists[0]
        for c, d in zip(kids[1:], dists[1:]):
            if d < best:                                        # strict: the first child wins ties
                best, final = d, c
        if ties is not None and dists.count(best) > 1:
            ties.append(1)
        if level == nid_level:
            nid = final
        if not voc.children[final]:
            break
    if nid is None:
        nid = final                                             # deviation 1: an early leaf is its own feature-vector node
    return voc.word_id[final], nid, voc.node_weight(final)


def transform(voc, feats, levelsup=0):
    """(words, values, fv, per_feature): ascending word ids, their L1-normalised values, fv = [(node id, [feature indices])] in ascending
    node id, per_feature = [(word, node, weight)] for every feature"""
    feats = np.asarray(feats, np.uint8).reshape(-1, 32)
    v, fv, per = {}, {}, []
    if voc.n_nodes == 0 or len(feats) == 0:
        return [], [], [], [(-1, 0, 0.0)] * len(feats)
    for i, f in enumerate(feats):
        word, nid, w = transform_feature(voc, f, levelsup)
        per.append((word, nid, w))
        if not w > 0:
            continue
        if voc.weighting in (TF_IDF, TF):
            v[word] = v[word] + w if word in v else w          # BowVector::addWeight
        else:
            v.setdefault(word, w)                               # BowVector::addIfNotExist
        fv.setdefault(nid, []).append(i)
    words = sorted(v)
    norm = 0.0
    for wd in words:                                            # std::map order
        norm += abs(v[wd])
    values = [v[wd] / norm if norm > 0.0 else v[wd] for wd in words]
    return words, values, [(n, fv[n]) for n in sorted(fv)], per


def l1_score(a_words, a_values, b_words, b_values):
    """L1Scoring::score of two normalised vectors: the merge walk over both maps"""
    b = dict(zip(b_words, b_values))
    score = 0.0
    for w, x in zip(a_words, a_values):
        if w in b:
            score += abs(x - b[w]) - abs(x) - abs(b[w])
    return -score / 2.0


class Database:
    def __init__(self, voc):
        self.voc = voc
        self.entries = []

    def add(self, feats):
        words, values, _, _ = transform(self.voc, feats)
        self.entries.append(dict(zip(words, values)))
        return len(self.entries) - 1

    def clear(self):
        self.entries = []

    def raw(self, feats, max_id=-1):
        """[(raw, entry id)] of the entries that share a word with the query, unordered"""
        words, values, _, _ = transform(self.voc, feats)
        out = []
        for e, ent in enumerate(self.entries):
            if max_id != -1 and e >= max_id:
                continue
            raw = None
            for w, q in zip(words, values):                     # ascending word id
                if w in ent:
                    t = abs(q - ent[w]) - abs(q) - abs(ent[w])
                    raw = t if raw is None else raw + t
            if raw is not None:
                out.append((raw, e))
        return out

    def query(self, feats, max_results=0, max_id=-1):
        res = sorted(self.raw(feats, max_id))                   # deviation 2: (raw, id)
        if max_results > 0:
            res = res[:max_results]
        return [(e, -raw / 2.0) for raw, e in res]


# ---------------------------------------------------------------- synthetic vocabularies and frames

def make_vocabulary(seed, k, L, weighting=TF_IDF, fewer=True, early_leaves=True, zero_weights=True, ties=True, scoring=L1_NORM):
    """A clustered tree in depth-first id order (so a node's children are NOT contiguous ids), with the edge cases planted:
    fewer     some inner nodes have fewer than k children
    early_leaves   some nodes above depth L are leaves
    zero_weights   about one word in eight weighs 0.0
    ties      the root's second child is two bits from the first (tie_probe() is one bit from both), and some siblings deeper down are copies"""
    rng = np.random.Generator(np.random.PCG64(seed))
    parent, leaf, desc, weight = [], [], [], []

    def flip(d, nbits):
        d = d.copy()
        for b in rng.choice(256, size=nbits, replace=False):
            d[b >> 3] ^= np.uint8(1 << (b & 7))
        return d

    def grow(pid, pdesc, depth):
        n = k
        if fewer and depth > 1 and rng.random() < 0.3:
            n = int(rng.integers(1, k))
        kids = []
        for c in range(n):
            d = rng.integers(0, 256, 32, dtype=np.uint8) if depth == 1 else flip(pdesc, max(2, 48 >> depth))
            if ties and c > 0 and depth > 1 and rng.random() < 0.25:
                d = kids[int(rng.integers(0, c))].copy()        # equal siblings: every feature ties between them
            if ties and depth == 1 and c == 1:
                d = kids[0].copy(); d[0] ^= np.uint8(3)          # two bits from the first child
            kids.append(d)
        for c in range(n):
            is_leaf = depth == L or (early_leaves and depth < L and rng.random() < 0.15)
            parent.append(pid); leaf.append(1 if is_leaf else 0); desc.append(kids[c])
            w = float(rng.uniform(0.05, 9.0))
            if zero_weights and is_leaf and rng.random() < 0.125:
                w = 0.0
            weight.append(w)
            nid = len(parent)
            if not is_leaf:
                grow(nid, kids[c], depth + 1)

    grow(0, None, 1)
    return Vocabulary(k, L, scoring, weighting, parent, leaf, np.array(desc, np.uint8).reshape(-1, 32), weight)


def tie_probe(voc):
    """one bit from the root's first child and one from its second: equal distances, the first must win"""
    d = voc.node_desc(voc.children[0][0]).copy()
    d[0] ^= np.uint8(1)
    return d


def make_features(voc, seed, n, random_share=0.2):
    """n descriptors near nodes of the tree (a few bits off) and some uniformly random ones; rows 0..2 are one descriptor three times
    (a word counted three times), row 3 the tie probe"""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = np.zeros((n, 32), np.uint8)
    for i in range(n):
        if rng.random() < random_share or voc.n_nodes == 0:
            out[i] = rng.integers(0, 256, 32, dtype=np.uint8)
        else:
            d = voc.desc[int(rng.integers(0, voc.n_nodes))].copy()
            for b in rng.choice(256, size=int(rng.integers(0, 4)), replace=False):
                d[b >> 3] ^= np.uint8(1 << (b & 7))
            out[i] = d
    if n >= 3:
        out[1] = out[0]; out[2] = out[0]
    if n >= 4 and voc.n_nodes >= 2:
        out[3] = tie_probe(voc)
    return out

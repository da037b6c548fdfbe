"""Helpers of the compact-proof tests: a Python model of the node rule, the word layout of a shard proof in either form and
the rebuilding of a container from shard proofs (the formats are csrc/proof.h)."""
import numpy as np

P = 2013265921
DVP1, DVP2, DVC3 = 0x31505644, 0x32505644, 0x33435644


def model_nodes(depth, indices):
    """The rule of the compact form: the (level, index) pairs listed for a tree of 2^depth leaves, in wire order."""
    keys = sorted({i % (1 << depth) for i in indices})
    out = []
    for s in range(depth, 0, -1):
        half = 1 << (s - 1)
        out += [(s, n ^ half) for n in keys if n ^ half not in keys]
        keys = sorted({n % half for n in keys})
    return out


def shard_layout(w):
    """w: the words of one shard proof.  -> dict(compact, head_end, queries_end, lists=[(count position, first digest word,
    end)]) with positions in words; a plain proof has no lists."""
    compact = int(w[0]) == DVP2
    assert compact or int(w[0]) == DVP1
    at = 1 + 24
    at += 1 + int(w[at])                       # public values
    nchips = int(w[at]); at += 1
    for _ in range(nchips):
        at += 6
        for _ in range(7):
            at += 1 + 4 * int(w[at])
    nfri = int(w[at]); at += 1 + 8 * nfri
    at += 4 + 1
    head_end = at
    nq = int(w[at]); at += 1
    for _ in range(nq):
        for _ in range(4):
            nm = int(w[at]); at += 1
            for _ in range(nm):
                at += 1 + int(w[at])
            if not compact:
                at += 1 + 8 * int(w[at])
        nl = int(w[at]); at += 1
        for _ in range(nl):
            at += 4
            if not compact:
                at += 1 + 8 * int(w[at])
    queries_end = at
    lists = []
    if compact:
        for _ in range(4 + nfri):
            n = int(w[at])
            lists.append((at, at + 1, at + 1 + 8 * n))
            at += 1 + 8 * n
    assert at == len(w), (at, len(w))
    return dict(compact=compact, head_end=head_end, queries_end=queries_end, lists=lists)


def container_parts(proof):
    """-> (head words of the container up to the first shard, [shard words])"""
    w = np.frombuffer(proof, np.uint32)
    assert int(w[0]) == DVC3
    n, pvl = int(w[1]), int(w[3])
    at = 4 + (pvl + 3) // 4
    head, shards = w[:at].copy(), []
    for _ in range(n):
        k = int(w[at])
        shards.append(w[at + 1:at + 1 + k].copy())
        at += 1 + k
    assert at == len(w)
    return head, shards


def container_join(head, shards):
    parts = [np.asarray(head, np.uint32)]
    for s in shards:
        parts += [np.array([len(s)], np.uint32), np.asarray(s, np.uint32)]
    return np.concatenate(parts).tobytes()


def bump(w, pos):
    """word pos + 1 mod p (a field word), or a count / length + 1"""
    w = w.copy()
    w[pos] = (int(w[pos]) + 1) % P if w[pos] < P else int(w[pos]) - 1
    return w


class Tree:
    """A natural-order Merkle tree of 2^depth random leaf digests built with the oracle's compression; where inject_at[lh]
    is set, every node of level lh is compressed once more with a digest of its own (the rows of shorter matrices)."""

    def __init__(self, oracle, rng, depth, inject_at=None):
        self.depth, self.oracle = depth, oracle
        self.inject_at = np.zeros(depth, np.uint8) if inject_at is None else np.asarray(inject_at, np.uint8)
        self.levels = [None] * (depth + 1)
        self.rows = [rng.integers(0, P, (1 << lh, 8), dtype=np.uint32) for lh in range(depth)]
        self.levels[depth] = rng.integers(0, P, (1 << depth, 8), dtype=np.uint32)
        for s in range(depth, 0, -1):
            half = 1 << (s - 1)
            up = np.zeros((half, 8), np.uint32)
            for j in range(half):
                up[j] = oracle.compress(self.levels[s][j], self.levels[s][j + half])
                if self.inject_at[s - 1]:
                    up[j] = oracle.compress(up[j], self.rows[s - 1][j])
            self.levels[s - 1] = up
        self.root = self.levels[0][0]

    def opening(self, indices):
        """what n queries carry: leaf digests [n][8], joining digests [depth][n][8], and the listed nodes"""
        d = self.depth
        idx = [i % (1 << d) for i in indices]
        leaf = np.stack([self.levels[d][i] for i in idx])
        inject = np.zeros((d, len(idx), 8), np.uint32)
        for lh in range(d):
            for q, i in enumerate(idx):
                inject[lh, q] = self.rows[lh][i % (1 << lh)]
        nodes = np.array([self.levels[s][i] for s, i in model_nodes(d, idx)], np.uint32).reshape(-1, 8)
        return leaf, inject, nodes

    def walk(self, indices, leaf, inject, nodes, root):
        """the host's walk in Python: equal digests where queries share a node, then level by level with the listed nodes"""
        d, comp = self.depth, self.oracle.compress
        cur = {}
        for q, i in enumerate(indices):
            if not np.array_equal(cur.setdefault(i % (1 << d), leaf[q]), leaf[q]):
                return False
        k = 0
        for s in range(d, 0, -1):
            half = 1 << (s - 1)
            listed = {}
            for n in sorted(cur):
                if n ^ half not in cur:
                    listed[n ^ half] = nodes[k]
                    k += 1
            up = {}
            for n in sorted(cur):
                j = n % half
                if j in up:
                    continue
                l = cur.get(j, listed.get(j))
                r = cur.get(j + half, listed.get(j + half))
                up[j] = comp(l, r)
                if self.inject_at[s - 1]:
                    mine = [inject[s - 1][q] for q, i in enumerate(indices) if i % half == j]
                    if any(not np.array_equal(mine[0], m) for m in mine):
                        return False
                    up[j] = comp(up[j], mine[0])
            cur = up
        return k == len(nodes) and np.array_equal(cur[0], root)

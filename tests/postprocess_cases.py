"""Crafted head bytes for the decode + NMS kernel and the coverage condition of every scenario (tests/test_postprocess_ref_host.py asserts
the conditions on the CPU, tests/test_gpu_postprocess.py runs the same frames on the GPU).  Every condition is computed from the numpy
reference's histogram, `visited`, `count` and round list (postprocess_ref.rounds) - never from the kernel under test.

The tool behind most scenarios is the CLUSTER generator: a K x K grid of target centres and one target size; every anchor gets the four
box bytes whose table entries bring its decoded box closest to the nearest target, and is dropped (class bytes -128) when any of the four
errors exceeds 2 % of the target size.  Boxes of one cluster then overlap almost fully and clusters are disjoint: with K * K <
max_detections the reference survives with exactly K * K boxes and VISITS EVERY CANDIDATE, so every position of every round's sort
bears on the output and every round and slice of the kernel has to run."""
import functools
from types import SimpleNamespace

import numpy as np

from postprocess_ref import POST_CAP, PostModel, postprocess_ref, rounds

LOW = -128
SIZES = (1, 255, 256, 257, 341, 342, 512, 513, 1023, 1024, 1025, 2047, 2048)

# per model kind: cluster grid / target size for the "visit everything" scenarios, the same for deep25, and which scenarios run
KINDS = {
    "lite0": dict(K=4, size=0.22, Kd=6, sized=0.15, sizes=SIZES,
                  names=("empty", "threshold", "sparse", "sizes", "bin2048", "bin2049", "plateau_all", "gap", "deep25", "low_plateau",
                         "mixed_ranks", "boundaries", "random")),
    "lite2": dict(K=4, size=0.22, sizes=(257, 1025, 2048),
                  names=("sizes", "plateau_all", "gap", "low_plateau", "mixed_ranks", "mixed_high", "boundaries")),
    "tiny": dict(K=3, size=0.3, names=("empty", "threshold", "sparse", "plateau_all", "full_rank", "mixed_ranks", "boundaries", "random")),
}
HIGH_ANCHOR = 20480     # anchors from here on lie beyond the kernel's five register slots per thread (5 x 1024 threads x 4 anchors)


class Gen:
    def __init__(self, m, kind):
        self.m, self.kind, self.cfg = m, kind, KINDS[kind]
        self.qual = np.nonzero(m.score >= m.thr)[0] - 128                  # qualifying class bytes, ascending
        u = np.unique(m.score[self.qual + 128])
        self.ranks = [self.qual[m.score[self.qual + 128] == s] for s in u]  # ascending score: the bytes of every plateau
        self._clusters = {}

    # ---- building blocks ---------------------------------------------------------------------------------------------------
    def blank(self, rng):
        m = self.m
        return np.full((m.A, m.C), LOW, np.int8), rng.integers(-128, 128, (m.A, 4)).astype(np.int8)

    def put(self, cls, rng, anchors, bytes_):
        """One candidate byte per anchor in a random column, the other columns stay at -128."""
        anchors = np.asarray(anchors, int)
        cls[anchors, rng.integers(0, self.m.C, len(anchors))] = np.asarray(bytes_, np.int8)

    def clusters(self, K, size, tol=0.02):
        """-> accepted anchors (ascending), their cluster ids, box bytes [A, 4] for every anchor."""
        if (K, size) not in self._clusters:
            m = self.m
            an = m.anchors.astype(np.float64)
            cent = (np.arange(K) + 0.5) / K
            iy, ix = np.argmin(np.abs(an[:, 0, None] - cent[None]), 1), np.argmin(np.abs(an[:, 1, None] - cent[None]), 1)

            def pick(tab, target):      # nearest table entry per anchor and its error
                j = np.argmin(np.abs(tab[None, :] - target[:, None]), 1)
                return j, np.abs(tab[j] - target)
            jy, ey = pick(m.dq, (cent[iy] - an[:, 0]) / an[:, 2])
            jx, ex = pick(m.dq, (cent[ix] - an[:, 1]) / an[:, 3])
            jh, eh = pick(m.ex, size / an[:, 2])
            jw, ew = pick(m.ex, size / an[:, 3])
            lim = tol * size
            ok = (ey * an[:, 2] < lim) & (ex * an[:, 3] < lim) & (eh * an[:, 2] < lim) & (ew * an[:, 3] < lim)
            box = (np.stack([jy, jx, jh, jw], 1) - 128).astype(np.int8)
            self._clusters[(K, size)] = (np.nonzero(ok)[0], (iy * K + ix)[ok], box)
        return self._clusters[(K, size)]

    def cluster_frame(self, rng, K=None, size=None):
        acc, cid, cbox = self.clusters(K or self.cfg["K"], size or self.cfg["size"])
        cls, box = self.blank(rng)
        box[acc] = cbox[acc]
        return cls, box, acc, cid

    def mid_plateau(self):
        """A class byte in the middle of the qualifying range (every `sizes`-like scenario parks its bulk there)."""
        return int(self.ranks[len(self.ranks) // 2][0])

    def high_bytes(self, n):
        """One byte of each of the n highest ranks."""
        return np.asarray([r[-1] for r in self.ranks[-n:]], np.int8)

    # ---- the scenarios: each -> [(name, cls, box, check)] ---------------------------------------------------------------
    def empty(self, rng):
        cls, box = self.blank(rng)
        cls[:] = rng.integers(-128, self.m.bmin, cls.shape).astype(np.int8)       # every byte below the threshold, the one just below too
        cls[::7] = self.m.bmin - 1

        def check(r, rd):
            assert r.n_cand == 0 and r.count == 0 and rd == []
        return [("empty", cls, box, check)]

    def threshold(self, rng):
        m = self.m
        cls, box = self.blank(rng)
        pick = rng.choice(m.A, 24, replace=False)
        self.put(cls, rng, pick[:12], np.full(12, m.bmin))
        self.put(cls, rng, pick[12:], np.full(12, m.bmin - 1))

        def check(r, rd):
            assert m.score[m.bmin + 128] >= m.thr > m.score[m.bmin - 1 + 128]
            assert sorted(r.order.tolist()) == sorted(pick[:12].tolist()) and r.visited == 12 and len(r.hist) == 1
        return [("threshold", cls, box, check)]

    def sparse(self, rng):
        m = self.m
        cls, box = self.blank(rng)
        n = min(40, len(self.ranks))
        self.put(cls, rng, rng.choice(m.A, n, replace=False), rng.permutation(self.high_bytes(n)))

        def check(r, rd):
            assert r.n_cand == n <= 40 and all(c == 1 for _, c in r.hist) and len(rd) == 1 and rd[0][0] == "count4"
        return [("sparse", cls, box, check)]

    def _head_and_plateau(self, rng, cls, chosen, head_n=200, head_ranks=20):
        """A head of `head_n` of the chosen anchors on `head_ranks` distinct high ranks, the rest on one plateau byte below them."""
        chosen = np.asarray(chosen)
        head = rng.choice(len(chosen), min(head_n, len(chosen)), replace=False)
        rest = np.setdiff1d(np.arange(len(chosen)), head)
        self.put(cls, rng, chosen[head], rng.choice(self.high_bytes(head_ranks), len(head)))
        self.put(cls, rng, chosen[rest], np.full(len(rest), self.mid_plateau()))

    def sizes(self, rng):
        out = []
        for N in self.cfg["sizes"]:
            cls, box, acc, _ = self.cluster_frame(rng)
            assert len(acc) >= N
            self._head_and_plateau(rng, cls, acc[-N:])
            want = "bitonic" if N > 1024 else f"count{min(1024 // N, 4)}"

            def check(r, rd, N=N, want=want):
                assert r.n_cand == N and r.count < self.m.maxdet and r.visited == N
                assert rd == [(want, N)], rd        # the head (<= 200 < 256 candidates) lets the plateau bin join the same round
            out.append((f"sizes{N}", cls, box, check))
        return out

    def _bin(self, rng, n):
        cls, box, acc, _ = self.cluster_frame(rng)
        assert len(acc) >= n + 5
        self.put(cls, rng, acc[-n:], np.full(n, self.mid_plateau()))
        self.put(cls, rng, acc[-n - 5:-n], self.high_bytes(5))
        return cls, box

    def bin2048(self, rng):
        cls, box = self._bin(rng, 2048)

        def check(r, rd):
            assert r.visited == r.n_cand == 2053 and r.count < self.m.maxdet
            assert rd == [("count4", 5), ("bitonic", 2048)], rd          # the largest unsliced round: no padding key
        return [("bin2048", cls, box, check)]

    def bin2049(self, rng):
        cls, box = self._bin(rng, 2049)

        def check(r, rd):
            assert r.visited == r.n_cand == 2054 and r.count < self.m.maxdet
            assert rd[0] == ("count4", 5) and all(k.startswith("slice:") for k, _ in rd[1:]) and sum(n for _, n in rd[1:]) == 2049, rd
            assert len(rd) == 1 + -(-self.m.A // POST_CAP)              # the smallest sliced bin: every slice of anchor indices is walked
        return [("bin2049", cls, box, check)]

    def plateau_all(self, rng):
        cls, box, acc, _ = self.cluster_frame(rng)
        self.put(cls, rng, acc, np.full(len(acc), self.mid_plateau()))
        oversized = self.kind != "tiny"       # the tiny models hold too few anchors for an oversized bin: one round in pure anchor order

        def check(r, rd):
            assert r.visited == r.n_cand == len(acc) and r.count < self.m.maxdet and len(r.hist) == 1
            assert r.order.tolist() == acc.tolist()
            if oversized:
                assert len(acc) > POST_CAP and len(rd) == -(-self.m.A // POST_CAP) and all(k.startswith("slice:") for k, _ in rd), rd
            else:
                assert len(rd) == 1 and len(acc) > 64, rd
        return [("plateau_all", cls, box, check)]

    def full_rank(self, rng):
        """Every anchor a candidate on ONE rank, its plateau byte in a random column and lower qualifying bytes in the others: the one
        oversized bin a model of 3 k anchors can hold, so that the slice walk and the bitonic network run behind every class-byte staging
        path (C = 1, 3, 4 exist only as tiny models)."""
        m = self.m
        p = self.mid_plateau()
        lower = self.qual[self.qual < p]
        cls = rng.choice(lower, (m.A, m.C)).astype(np.int8)
        cls[np.arange(m.A), rng.integers(0, m.C, m.A)] = p
        box = rng.integers(-128, 128, (m.A, 4)).astype(np.int8)

        def check(r, rd):
            assert r.n_cand == m.A > POST_CAP and len(r.hist) == 1 and rd[0] == ("slice:bitonic", POST_CAP), rd
            got = set(r.classes[:r.count].astype(int).tolist())
            assert r.count == m.maxdet and got == set(range(m.C)), got
        return [("full_rank", cls, box, check)]

    def gap(self, rng):
        m = self.m
        cls, box = self.blank(rng)
        box[:, 2:] = 127
        p = self.mid_plateau()
        cls[0:9, m.C - 1] = p
        cls[6000:, 0] = p

        def check(r, rd):
            sel = np.asarray(r.selected)
            assert (sel >= 4096).any() and (sel < 2048).any() and not ((r.order >= 2048) & (r.order < 4096)).any()
            assert rd[0] == ("slice:count4", 9) and rd[1] == ("slice:empty", 0) and rd[2][1] > 0, rd      # the n == 0 round, then on
        return [("gap", cls, box, check)]

    def deep25(self, rng):
        cls, box, acc, _ = self.cluster_frame(rng, self.cfg["Kd"], self.cfg["sized"])
        self.put(cls, rng, acc, np.full(len(acc), self.mid_plateau()))

        def check(r, rd):
            assert r.count == self.m.maxdet and r.selected[-1] >= POST_CAP and r.visited < r.n_cand
            assert len(rd) >= 2 and len(rd) < -(-self.m.A // POST_CAP), rd     # the kernel stops inside a later slice, before the last
        return [("deep25", cls, box, check)]

    def low_plateau(self, rng):
        m = self.m
        cls, box, acc, _ = self.cluster_frame(rng)
        low = self.qual[:len(self.ranks[0]) + 16]                  # the lowest plateau's bytes and the 16 bytes above them
        self.put(cls, rng, acc, rng.choice(low, len(acc)))

        def check(r, rd):
            big = max(c for _, c in r.hist)
            assert big > POST_CAP and r.hist[0][1] != big and r.hist[-1][1] == big        # oversized, and the LOWEST rank, not the top
            assert r.visited == r.n_cand and r.count < m.maxdet
            assert not rd[0][0].startswith("slice:") and rd[-1][0].startswith("slice:"), rd
        return [("low_plateau", cls, box, check)]

    def _mixed(self, rng, name, lo_anchor=0):
        """Every column of every accepted anchor random over the whole qualifying range.  In the first clusters the lowest accepted anchor
        leads its cluster on the highest plateau of several bytes, one byte of it in column w and ANOTHER byte of it in the columns
        behind w, every other anchor of the cluster below that plateau: the survivor's class must be w, the first column."""
        m = self.m
        cls, box, acc, cid = self.cluster_frame(rng)
        keep = acc >= lo_anchor
        acc, cid = acc[keep], cid[keep]
        cls[acc] = rng.choice(self.qual, (len(acc), m.C)).astype(np.int8)
        multi = [r for r in self.ranks if len(r) >= 2][-1]
        below = self.qual[m.score[self.qual + 128] < m.score[multi[0] + 128]]
        leads = {}
        for j, c in enumerate(np.unique(cid)[:max(m.C, 2) + 2]):
            mine = acc[cid == c]
            cls[mine] = rng.choice(below, (len(mine), m.C)).astype(np.int8)
            w = j % m.C
            cls[mine[0], :w] = below[0]
            cls[mine[0], w] = multi[-1]
            cls[mine[0], w + 1:] = multi[0]
            leads[int(mine[0])] = w

        def check(r, rd):
            assert r.visited == r.n_cand == len(acc) and r.count < m.maxdet
            assert min(r.order) >= lo_anchor
            got = dict(zip(r.selected, r.classes[:r.count].astype(int).tolist()))
            assert all(got.get(a) == w for a, w in leads.items()), (got, leads)      # the leads survive, first column wins
            assert set(got.values()) == set(range(m.C))                              # every column wins somewhere
            if m.C > 1:
                assert any(len(set(cls[a].tolist())) > 1 and (m.score[cls[a].astype(int) + 128] == r.scores[i]).sum() > 1
                           for i, a in enumerate(r.selected))                        # two different bytes, one score, on a survivor
            if self.kind == "tiny":       # about 160 accepted anchors: one round on many ranks
                assert len(r.hist) > 16 and len(rd) == 1, (len(r.hist), rd)
            else:
                assert len(r.hist) > 64 and len(rd) > 2, (len(r.hist), rd)
        return [(name, cls, box, check)]

    def mixed_ranks(self, rng):
        return self._mixed(rng, "mixed_ranks")

    def mixed_high(self, rng):
        return self._mixed(rng, "mixed_high", HIGH_ANCHOR)

    def boundary_anchors(self):
        m = self.m
        s = {m.A - 1, m.A - 2}
        for l in range(m.nl):
            s |= {int(m.base[l]), int(m.base[l + 1]) - 1}
            if m.base[l] & 3:                                     # the dword that straddles the level start
                s |= set(range(int(m.base[l]) & ~3, (int(m.base[l]) & ~3) + 4))
        for a in range(4096, m.A, 4096):                          # the stride between a thread's dwords
            s |= {a - 1, a}
        return np.asarray(sorted(a for a in s if 0 <= a < m.A))

    def boundaries(self, rng, n=1):
        out = []
        pick = self.boundary_anchors()
        for i in range(n):
            cls, box = self.blank(rng)
            hb = self.high_bytes(min(30, len(self.ranks)))
            for c in range(self.m.C):                             # every column random and high: the per-column maximum at every boundary
                cls[pick, c] = rng.choice(hb, len(pick))

            def check(r, rd):
                assert sorted(r.order.tolist()) == pick.tolist() and len(rd) == 1
            out.append((f"boundaries{i}", cls, box, check))
        return out

    def random(self, rng, n=3):
        out = []
        for i in range(n):
            cls = rng.integers(-128, 128, (self.m.A, self.m.C)).astype(np.int8)
            box = rng.integers(-128, 128, (self.m.A, 4)).astype(np.int8)

            def check(r, rd):
                assert r.n_cand > self.m.A // 8 and r.count > 0
            out.append((f"random{i}", cls, box, check))
        return out


@functools.lru_cache(maxsize=None)
def build(path, kind, seed=1):
    """-> (PostModel, [case]): case.name, .cls [A, C], .box [A, 4], .ref (postprocess_ref), .rounds, .check() (the coverage condition).
    The list ends with eight `boundaries` frames of different seeds: a batch of its own, one per frame slot."""
    m = PostModel(path)
    g = Gen(m, kind)
    rng = np.random.default_rng(seed)
    raw = []
    for name in KINDS[kind]["names"]:
        raw += g.boundaries(rng, 8) if name == "boundaries" else getattr(g, name)(rng)
    cases = []
    for name, cls, box, check in raw:
        cls.setflags(write=False)
        box.setflags(write=False)
        r = postprocess_ref(m, cls, box)
        rd = rounds(m, r)
        cases.append(SimpleNamespace(name=name, cls=cls, box=box, ref=r, rounds=rd, check=functools.partial(check, r, rd)))
    return m, cases


def model_files(tmpdir, model_lite0):
    """-> {name: (container path, kind)} of the six models: the two committed ones and TinyModel(S=32, num_classes=C), C = 1..4, written
    by the independent encoder of tests/tflite_minienc.py and imported (the importer takes every C the container format allows)."""
    import os
    from tflite_minienc import TinyModel
    from vbt_amd.tflite_import import convert
    out = {"lite0": (model_lite0, "lite0"), "lite2": (os.path.join(os.path.dirname(model_lite0), "efficientdet_lite2_synth.vbtm"), "lite2")}
    for C in (1, 2, 3, 4):
        tfl, vb = os.path.join(str(tmpdir), f"tiny_c{C}.tflite"), os.path.join(str(tmpdir), f"tiny_c{C}.vbtm")
        with open(tfl, "wb") as f:
            f.write(TinyModel(S=32, seed=5, num_classes=C).build().serialize())
        convert(tfl, vb)
        out[f"tiny_c{C}"] = (vb, "tiny")
    return out


MODELS = ("lite0", "lite2", "tiny_c1", "tiny_c2", "tiny_c3", "tiny_c4")


def describe(case):
    """One line for a coverage table: candidates, visited, count and the round kinds."""
    kinds = {}
    for k, _ in case.rounds:
        kinds[k] = kinds.get(k, 0) + 1
    return f"{case.name}: candidates {case.ref.n_cand}, visited {case.ref.visited}, count {case.ref.count}, rounds " + \
        (", ".join(f"{v} x {k}" for k, v in kinds.items()) or "none")

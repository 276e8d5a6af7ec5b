"""The inputs of the `fingerprint` / `repeat` kernels, shared by tests/test_repeat_ref.py (which proves on the restatement alone what
they reach) and tests/test_gpu_repeat.py (which runs them).  The shapes are the smallest at which the kernels can still go wrong."""
import collections
import zlib

import numpy as np

from pyannote_video_amd import repeat as _repeat

S = _repeat.RUNS_STRIP         # PVF_RUNS_STRIP: rows of A a workgroup of print_runs_k walks (strip seams at its multiples)
GROUP = 256                    # diagonals of a workgroup (group seams at d0 + its multiples)
PLANT_BITS = 6                 # the distance of a planted copy that is not exact
TAU_RANDOM = 10                # random rows never come this close (tests/test_repeat_ref.py)

# ---- frames -------------------------------------------------------------------------------------------------------------------------
SIZES = ((1, 1), (8, 8), (9, 9), (10, 7), (64, 36), (641, 359), (1920, 1080))       # (w, h); 3 w is no multiple of 4 at 1, 9, 641
BIG_SIZE = (3840, 2160)
CONTENTS = ("zeros", "full", "ramp_x", "ramp_y", "checker", "noise")


def make_frame(w, h, content, seed=0):
    """uint8 [h, w, 3], a function of the arguments alone"""
    if content == "zeros":
        return np.zeros((h, w, 3), np.uint8)
    if content == "full":
        return np.full((h, w, 3), 255, np.uint8)
    i, j, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    if content == "ramp_x":                  # rises along every row: over 9 columns or more the grid's luma rises strictly
        return ((j * 255) // max(w - 1, 1) + 0 * c).astype(np.uint8)
    if content == "ramp_y":
        return ((i * 255) // max(h - 1, 1) + 0 * c).astype(np.uint8)
    if content == "checker":                 # saturated, seven cells a side: the nine grid cells straddle them
        return ((((i * 7) // h + (j * 7) // w) & 1) * 255 + 0 * c).astype(np.uint8)
    rng = np.random.default_rng(zlib.crc32(("%d %d %d" % (w, h, seed)).encode()))
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---- tables and planted runs ---------------------------------------------------------------------------------------------------------
def random_prints(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 64, (n, 2), dtype=np.uint64)


def flipped(rows, bits, seed):
    """the rows with exactly `bits` of their 128 bits flipped"""
    rng = np.random.default_rng(seed)
    out = np.array(rows, np.uint64)
    for r in range(len(out)):
        for k in rng.choice(128, bits, replace=False):
            out[r, k // 64] ^= np.uint64(1 << (int(k) % 64))
    return out


Plant = collections.namedtuple("Plant", "i j n bits what")
RunCase = collections.namedtuple("RunCase", "name A ua B ub plants")        # B None: self mode


def planted(name, NA, NB, plants, seed):
    """random tables with B[j .. j + n) = A[i .. i + n) with `bits` flipped bits a row, for every plant (their B ranges are disjoint)"""
    A, B = random_prints(NA, seed), random_prints(NB, seed + 1)
    taken = np.zeros(NB, bool)
    for k, p in enumerate(plants):
        assert 0 <= p.i and p.i + p.n <= NA and 0 <= p.j and p.j + p.n <= NB and not taken[p.j:p.j + p.n].any(), p
        taken[p.j:p.j + p.n] = True
        B[p.j:p.j + p.n] = flipped(A[p.i:p.i + p.n], p.bits, seed + 10 + k)
    return RunCase(name, A, np.ones(NA, np.uint8), B, np.ones(NB, np.uint8), tuple(plants))


SEAM_NA, SEAM_NB = 3 * S + 300, 3 * S + 500


def seam_case():
    """every place a run can lie with respect to the kernel's tiles, in one pair of tables over three strips and a bit"""
    NA, NB = SEAM_NA, SEAM_NB
    d0 = -(NA - 1)

    def on_group(k, lane, i, n, bits, what):          # a run on diagonal d0 + 256 k + lane, from row i
        return Plant(i, i + d0 + GROUP * k + lane, n, bits, what)
    k = (NA - 1) // GROUP + 1                          # the first group of diagonals that lies at d > 0
    return planted("seams", NA, NB, [
        Plant(0, 40, 7, 0, "touches row 0 of A"),
        Plant(NA - 1, 0, 1, 0, "the first diagonal; row 0 of B and the last row of A"),
        Plant(0, NB - 1, 1, PLANT_BITS, "the last diagonal; the last row of B"),
        Plant(NA - 6, 100, 6, PLANT_BITS, "ends on the last row of A"),
        Plant(200, NB - 10, 4, PLANT_BITS, "length 4"),
        Plant(S - 1, 500, 3, PLANT_BITS, "starts on the last row of a strip"),
        Plant(S, 600, 3, 0, "starts on the first row of a strip"),
        Plant(2 * S - 5, 700, 10, PLANT_BITS, "crosses one seam"),
        Plant(S - 3, 1000, 2 * S + 10, PLANT_BITS, "crosses three seams"),
        on_group(k, 0, 100, 4, PLANT_BITS, "the first diagonal of a group"),
        on_group(k, GROUP - 1, 350, 5, 0, "the last diagonal of a group"),
    ], seed=100)


def self_case():
    """one table against itself: a copy further on, a copy across the strip seam, and a frozen stretch (equal neighbours)"""
    N = S + 300
    A = random_prints(N, 300)
    A[400:405] = flipped(A[10:15], PLANT_BITS, 301)             # (10, 400, 5)
    A[S + 100:S + 106] = A[S - 2:S + 4]                         # (S - 2, S + 100, 6): crosses the seam
    A[50:58] = A[50]                                            # frozen: (50, 50 + g, 8 - g) on every diagonal g = 1 .. 7
    plants = (Plant(10, 400, 5, PLANT_BITS, "a copy"), Plant(S - 2, S + 100, 6, 0, "a copy across the seam")) + \
        tuple(Plant(50, 50 + g, 8 - g, 0, "frozen") for g in range(1, 8))
    return RunCase("self", A, np.ones(N, np.uint8), None, None, plants)


EDGE_SIZES = (1, 2, 255, 256, 257, 511, 512, 513, S - 1, S, S + 1)
SIZE_PAIRS = ((1, 1), (1, 2), (2, 1), (2, 2), (1, 257), (257, 1), (255, 256), (256, 255), (256, 257), (257, 256), (511, 513), (512, 512),
              (513, 511), (S - 1, S + 1), (S, S), (S + 1, S - 1), (S + 1, 2), (2, S + 1), (1, S), (S, 1))
THIN = ((3, 5000), (5000, 3))


def size_case(NA, NB):
    """random tables of this size with one exact copy as long as fits (at most 5), ending in the last cell of both"""
    n = min(NA, NB, 5)
    return planted("size %d x %d" % (NA, NB), NA, NB, [Plant(NA - n, NB - n, n, 0, "ends in the corner")], seed=1000 + 7 * NA + NB)


def all_equal(NA, NB):
    """every print the same: every diagonal is one run"""
    A = np.tile(random_prints(1, 77), (NA, 1))
    return RunCase("equal %d x %d" % (NA, NB), A, np.ones(NA, np.uint8), np.tile(A[:1], (NB, 1)), np.ones(NB, np.uint8), ())

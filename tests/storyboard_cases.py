"""The cases of the thumbnail kernel, shared by tests/test_storyboard_ref.py (which proves on the restatement alone what the table
reaches) and tests/test_gpu_storyboard.py (which runs them).  The shapes are the smallest at which frame_thumbs_k can still go wrong."""
import collections
import zlib

import numpy as np

# ---- the seams frame_thumbs_k declares (csrc/board.hip) -----------------------------------------------------------------------------
SEG_PX = 85                # TB_SEG_PX: output columns of a block (column segments)
PIECE_COLS = 1024          # TB_PIECE_COLS: source columns a block stages at a time (LDS pieces)
LDS_BYTES = 20480          # TB_LDS: the staged rows of a piece


def stage_rows(ncols):
    """source rows of a piece of ncols columns that are staged at a time (row bands): TB_LDS / pitch"""
    return LDS_BYTES // ((3 * ncols + 30) & ~15)


def block_columns(w, tw, seg):
    """the source columns [J0, J1) of column segment `seg`"""
    X0, X1 = seg * SEG_PX, min((seg + 1) * SEG_PX, tw)
    return (X0 * w) // tw, (X1 * w + tw - 1) // tw


def row_count(h, th, Y):
    """source rows that output row Y touches"""
    return ((Y + 1) * h + th - 1) // th - (Y * h) // th


Case = collections.namedtuple("Case", "name w h tw th content")
CONTENTS = ("noise", "zeros", "full", "checker", "ramp")


def make_frame(case):
    """uint8 [h, w, 3], a function of the case alone"""
    w, h = case.w, case.h
    if case.content == "zeros":
        return np.zeros((h, w, 3), np.uint8)
    if case.content == "full":
        return np.full((h, w, 3), 255, np.uint8)
    i, j, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    if case.content == "checker":            # saturated, period 1
        return (((i + j) & 1) * 255).astype(np.uint8)
    if case.content == "ramp":               # neighbours differ by one: a 2 : 1 mean along x lands on .5
        return ((j + 3 * c + 7 * (i // 2)) % 256).astype(np.uint8)
    rng = np.random.default_rng(zlib.crc32(("%d %d" % (w, h)).encode()))
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


ALIGN_HEIGHTS = (1, 2, 3, 7, 8, 9)
RATIOS = (((17, 13), (5, 4)), ((64, 48), (7, 5)), ((65, 33), (64, 32)), ((3, 2), (8, 5)), ((255, 256), (1, 1)), ((341, 86), (160, 40)),
          ((1, 1), (1024, 1024)), ((1024, 3), (1, 1024)))
BIG = Case("sum64", 4105, 4105, 1, 1, "full")       # w h = 16 851 025 > 2^32 / 255: run by the GPU test on its own, every byte 255
BIG_TARGETS = ((1, 1), (3, 2))


def cases():
    out = []
    # row alignment: rows are 3 w bytes apart; with 17 rows every start alignment a width allows occurs
    for w in range(1, 18):
        for tw in (max(1, w // 2), w, 2 * w + 1):
            for th in ALIGN_HEIGHTS:
                out.append(Case("align", w, 17, tw, th, "noise"))
    for (w, h), (tw, th) in RATIOS:
        out.append(Case("ratio", w, h, tw, th, "noise"))
    # reducing, keeping and enlarging on each axis independently
    for tw in (5, 12, 29):
        for th in (4, 10, 23):
            out.append(Case("axes", 12, 10, tw, th, "noise"))
    # column segments: one below, on and above SEG_PX and 2 SEG_PX output columns, enlarging and reducing
    for tw in (SEG_PX - 1, SEG_PX, SEG_PX + 1, 2 * SEG_PX - 1, 2 * SEG_PX, 2 * SEG_PX + 1):
        out.append(Case("segment", 100, 5, tw, 2, "noise"))
        out.append(Case("segment", 301, 4, tw, 3, "noise"))
    # LDS pieces: a block whose source columns are one below, on and above PIECE_COLS and 2 PIECE_COLS
    for w in (PIECE_COLS - 1, PIECE_COLS, PIECE_COLS + 1, 2 * PIECE_COLS - 1, 2 * PIECE_COLS, 2 * PIECE_COLS + 1):
        out.append(Case("piece", w, 3, 1, 2, "noise"))
    out.append(Case("piece", 2 * PIECE_COLS + 1, 2, 2, 1, "noise"))
    # row bands: an output row of one below, on and above stage_rows source rows, for the widest piece (6) and a narrow one
    R = stage_rows(PIECE_COLS)
    for h in (R - 1, R, R + 1, 2 * R, 2 * R + 1):
        out.append(Case("band", PIECE_COLS, h, 1, 1, "noise"))
    R = stage_rows(5)
    for h in (R - 1, R, R + 1):
        out.append(Case("band", 5, h, 2, 1, "noise"))
    # contents
    for content in CONTENTS:
        out.append(Case("content", 37, 23, 5, 4, content))
        out.append(Case("content", 16, 16, 8, 16, content))
        out.append(Case("content", 6, 5, 13, 11, content))
    return out

"""CPU check of the step kernel's three-cell line table (csrc/g2048_core.h: line3_entry, line3_append,
board_move_lean3) through a TEST-ONLY host build (tests/native/line3_host.cpp).

The 16 KiB table over cells 0..2 plus the append step for cell 3 must equal line_move_left and
line_max_merge_field on every 16-bit line, and board_move_lean3 must equal board_move_lean (the 160 KiB tables) in
the board, in every summary field and in nzg.  Not a parity claim for the GPU path (tests/test_gpu_step_line3.py).
"""
import ctypes
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "rl-2048-with-reinforce-and-actor-critic_amd", "csrc")


@pytest.fixture(scope="module")
def l3():
    so = os.path.join(NATIVE, "libline3_host.so")
    src = os.path.join(NATIVE, "line3_host.cpp")
    hdr = os.path.join(CSRC, "g2048_core.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        tmp = f"{so}.{os.getpid()}.tmp"   # build aside, then rename: parallel workers never load a partial file
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-o", tmp, src], check=True)
        os.replace(tmp, so)
    L = ctypes.CDLL(so)
    for name, args in (("l3_check_entries", []), ("l3_check_lines", []), ("l3_check_slots", [ctypes.c_uint64]),
                       ("l3_check_random", [ctypes.c_int64, ctypes.c_uint64]), ("l3_check_board", [ctypes.c_uint64])):
        getattr(L, name).restype = ctypes.c_int64
        getattr(L, name).argtypes = args
    L.l3_overflow.restype = ctypes.c_uint32
    L.l3_overflow.argtypes = [ctypes.c_uint64, ctypes.c_uint32]
    return L


def _board(rows):
    """rows: four lists of four exponents, row r cell c -> nibble 4 r + c."""
    b = 0
    for r, row in enumerate(rows):
        for c, e in enumerate(row):
            b |= e << (4 * (4 * r + c))
    return b


def test_entries_match_their_definition(l3):
    """All 4,096 entries: r = line_move_left(o3), m = the last tile unless it is a merge product (then 16),
    f = line_max_merge_field(o3), sh = 4 * tiles(r), nothing above bit 29."""
    assert l3.l3_check_entries() == 0


def test_every_line(l3):
    """Entry + append == line_move_left and line_max_merge_field on all 65,536 lines (15+15 included: the nibble
    stays 15, the field is 15)."""
    assert l3.l3_check_lines() == 0


def test_every_line_in_every_slot(l3):
    """board_move_lean3 == board_move_lean: every 16-bit line value in each of the four line slots (the other
    lines random), under all four actions."""
    assert l3.l3_check_slots(0x2052) == 0


def test_random_boards(l3):
    """... on 200,000 random boards with exponents up to 15."""
    assert l3.l3_check_random(200_000, 0x2053) == 0


def test_saturated_lines(l3):
    """Boards with two and four 15-tiles in one line (the line_merges fallback), in every line slot and in both
    orientations, beside lines that merge without saturating."""
    lines = sorted(set(itertools.permutations([15, 15, 0, 14]))) + [(15, 15, 15, 15)]
    lines += [(15, 15, 14, 14), (14, 14, 15, 15), (15, 0, 15, 3), (3, 15, 0, 15), (15, 15, 15, 0), (0, 15, 15, 15)]
    other = [[1, 1, 2, 2], [3, 0, 3, 0], [0, 0, 0, 0], [5, 6, 7, 8]]
    took_fallback = 0
    for line in lines:
        for slot in range(4):
            rows = [list(r) for r in other]
            rows[slot] = list(line)
            for b in (_board(rows), _board([list(c) for c in zip(*rows)])):    # as a row, and as a column
                assert l3.l3_check_board(b) == 0, hex(b)
                took_fallback += sum(l3.l3_overflow(b, a) for a in range(4))
    assert took_fallback > 0

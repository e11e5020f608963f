"""The sparse line reference of tests/_lines_sparse.py against the dense rules of the suite, on real arrays of a few KiB: the scene
kinds that tests/test_gpu_lines_grids.py plants into gigabytes, built here at 64 bytes per tile.  For all twelve (how, inverted)
combinations the records worked out from the scene list alone must equal what tests/test_gpu_inverted.py's ref_inverted (for w and x,
tests/test_gpu_bounded.py's ref_lines / ref_kept; for the plain call, tests/test_gpu_lines.py's ref_lines) gives on the array.  No GPU."""
import numpy as np

from _lines_sparse import (BORDER_KINDS, FILLER, HOWS, KINDS, NL, Grid, background_scenes, border_scenes, checked, mixed, sparse_lines,
                           two_tile_scenes, write_scenes)
from test_gpu_bounded import ref_kept, ref_lines as ref_bounded_lines
from test_gpu_inverted import ref_inverted
from test_gpu_lines import ref_lines as ref_plain_lines

NEEDLE = b"qzjx"
LONG = b"quite a long needle, 33 bytes: qz"


def dense_of(scenes, length):
    return write_scenes(np.full(length, FILLER, dtype=np.uint8), scenes)


def agree(scenes, length, needle, delim=10, what=""):
    """all twelve combinations; returns {(how, inverted): number of selected lines}"""
    host = dense_of(scenes, length)
    sizes = {}
    for how in HOWS:
        sel, hit, every = ref_inverted(host, needle, delim, how)
        for inverted, want in ((False, hit), (True, sel)):
            got = sparse_lines(scenes, length, needle, delim, how, inverted)
            for g, w, name in zip(got, want, ("begin", "end", "number")):
                assert g.dtype == np.int64 and g.size == w.size and (g == w).all(), (what, how, inverted, name, g[:8], w[:8])
            sizes[how, inverted] = got[0].size
        assert sizes[how, False] + sizes[how, True] == every[0].size, (what, how)
    # the rules the dense reference is made of, taken directly
    for g, w in zip(sparse_lines(scenes, length, needle, delim, "", False), ref_plain_lines(host, needle, delim)):
        assert (g == w).all(), what
    for how, line, nocase in (("w", False, False), ("x", True, False), ("wi", False, True), ("xi", True, True)):
        want = ref_bounded_lines(host, needle, delim, line, nocase)
        assert ref_kept(host, needle, nocase, line, delim).size >= want[0].size
        for g, w in zip(sparse_lines(scenes, length, needle, delim, how, False), want):
            assert g.size == w.size and (g == w).all(), (what, how)
    return sizes


def small_grid(tile, n, nwg, shift):
    ntiles = 2 * nwg - 1
    length = ntiles * tile + shift - 7 + n - 1               # (the last tile is short, as where the view ends inside one)
    return Grid(length, tile, 2, ntiles, shift)


def test_the_tile_border_scenes_at_64_bytes_per_tile():
    seen = {}
    for rot in range(6):                                      # (the kinds walk their variants: every rotation shifts which come first)
        for shift in (0, 5):
            grid = small_grid(64, len(NEEDLE), 34, shift)
            assert grid.length < 5 * 1024
            long_line = (12 + rot, 19 + rot, 15 + rot)
            wgs = [w for w in range(grid.nwg) if not long_line[0] - 1 <= w <= long_line[1]]
            notes = {}
            scenes = two_tile_scenes(grid, NEEDLE, wgs[rot % 3:], long_line, notes)
            assert scenes[-1][0] + len(scenes[-1][1]) == grid.length           # flush with the end
            assert (scenes[0][0] == 0) == (rot % 3 == 0)                        # a scene at offset 0 when workgroup 0 is chosen
            sizes = agree(scenes, grid.length, NEEDLE, what=("tile 64", rot, shift))
            assert len(set(sizes[how, False] for how in HOWS)) >= 4, sizes
            assert all(0 < sizes[how, True] < sizes[how, False] + sizes[how, True] for how in HOWS), sizes
            for k, v in notes["uses"].items():
                seen[k] = seen.get(k, 0) + v
            # the long line is one record of the plain call: from its opening delimiter to its closing one, 7 workgroups on
            b, e, _ = sparse_lines(scenes, grid.length, NEEDLE, 10, "", False)
            span = e - b
            assert span.max() > 7 * 2 * 64 - 64 and int((span > 2 * 64).sum()) == 1, span.max()
    assert sorted(seen) == list(range(len(KINDS))) and min(seen.values()) >= 12, seen


def test_a_needle_verified_in_memory_and_other_delimiters():
    for needle, tile in ((LONG, 512), ((b"xyz" * 20)[:50], 1024)):
        grid = small_grid(tile, len(needle), 24, 0)
        long_line = (8, 14, 11)
        wgs = [w for w in range(grid.nwg) if not 7 <= w <= 14]
        scenes = two_tile_scenes(grid, needle, wgs, long_line)
        sizes = agree(scenes, grid.length, needle, what=("long", tile))
        assert len(set(sizes[how, False] for how in HOWS)) >= 4, sizes
    # the delimiter an upper-case letter that folds onto a needle byte; a blank; a needle that holds the delimiter
    grid = small_grid(64, 4, 20, 0)
    scenes = two_tile_scenes(grid, NEEDLE, range(grid.nwg))
    for delim in (ord("Q"), ord(" "), ord("k"), ord("q")):
        agree(scenes, grid.length, NEEDLE, delim, ("delimiter", delim))


def test_the_border_scenes_and_scenes_that_touch():
    n = len(NEEDLE)
    for tpw in (1, 2):
        grid = Grid(40 * 64 * tpw + n - 8, 64, tpw, 40 * tpw, 0)
        for rot in range(len(BORDER_KINDS)):
            scenes = background_scenes(grid, NEEDLE, (0, 3, 11, 12, 30, 39))
            for j, w in enumerate((8, 16, 24, 32)):
                scenes += border_scenes((j + rot) % len(BORDER_KINDS), grid.start(w), NEEDLE)
            scenes.append((grid.length - n - 1, NL + NEEDLE))
            sizes = agree(checked(scenes, grid.length), grid.length, NEEDLE, what=("borders", tpw, rot))
            assert 0 < sizes["", False] and 0 < sizes["", True]
    length = 1000
    touching = [
        [(0, NEEDLE + NL)],                                                   # offset 0, and nothing else
        [(0, NEEDLE[:2]), (2, NEEDLE[2:] + b"k" + NL), (7, NEEDLE), (7 + n, NL)],       # an occurrence cut by two scenes that touch
        [(100, NL + NEEDLE[:1]), (102, NEEDLE[1:] + NL), (102 + n, mixed(NEEDLE)), (102 + 2 * n, b" " + NEEDLE)],
        [(500, NL), (501, NEEDLE), (501 + n, NEEDLE), (501 + 2 * n, NL), (length - n, NEEDLE)],         # glued copies; flush, open
        [(length - n - 2, NL + NEEDLE + NL)],                                 # a delimiter on the last byte: no line behind it
        [(length - 1, NL)], [(0, NL)], [(0, NL), (1, NL), (length - 2, NL), (length - 1, NL)],
        [(300, NEEDLE)], [],                                                  # one unterminated line, with and without a match
        [(10, NEEDLE[:-1]), (10 + n + 4, NEEDLE[1:])],                        # near copies only: closer than the widening, no match
    ]
    for k, scenes in enumerate(touching):
        agree(checked(scenes, length), length, NEEDLE, what=("touching", k))
    # ignoring case, a delimiter 'Q' folds onto the needle's first byte: the copy that holds it is cut in two and matches no line
    sizes = agree([(100, b"QkkQzJx k"), (200, b"Q" + NEEDLE + b"Q")], length, NEEDLE, ord("Q"), "a delimiter that folds onto a needle byte")
    assert sizes["i", False] == 1 and sizes["i", True] == 4
    # a view as short as the needle, and shorter
    agree([(0, NEEDLE)], n, NEEDLE, what="the needle alone")
    agree([(0, NEEDLE[:3])], 3, NEEDLE, what="shorter than the needle")

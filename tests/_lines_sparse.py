"""Scenes on a haystack of one filler byte, and the line rule worked out from the scenes alone (a helper of tests/test_gpu_lines_grids.py
and tests/test_lines_sparse_cpu.py, not a test module).

A SCENE is a short byte string at a known offset; everything between the scenes is FILLER, which is no word byte, no letter, no
delimiter and no byte of the needle.  The builders place scenes where the line scans carry state - the tile border inside a
two-tile workgroup, a workgroup's end, the border between two chunks of parts - for a tile size that is a parameter, so that the same
scene kinds fit into a few KiB at 64 bytes per tile and into gigabytes at 16 KiB.  They return the list ``[(offset, bytes), ...]``.

The REFERENCE (`sparse_lines`) sees only that list, never the haystack: delimiters come from the scenes, occurrences from each
group of neighbouring scenes widened by len(needle) filler bytes on both sides, neighbour bytes from the same text (absent only at the
view's ends).  tests/test_lines_sparse_cpu.py holds it against the dense rules of the suite on real arrays; that is what allows it to
stand in for them on haystacks of gigabytes."""
import numpy as np

FILLER = 0x2E                                   # '.'
NL = b"\n"
HOWS = ("", "i", "w", "x", "wi", "xi")          # i: ignore case, w: whole word, x: whole line
_WORD = frozenset(b"0123456789_ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz")
KINDS = ("match in the first tile, line closes in the second", "delimiter on the first tile's last byte, match behind it",
         "delimiter on the second tile's first byte", "occurrence straddles the tile border",
         "line opens in the second tile with its match, closes in the next workgroup",
         "line opens in the second tile, its match is in the next workgroup", "line without a match across the tile border",
         "occurrence ends on the first tile's last byte; right neighbour a word byte, a blank, the delimiter",
         "occurrence begins on the second tile's first byte; left neighbour a word byte, a blank, the delimiter",
         "copies in mixed case")
BORDER_KINDS = ("match in front", "match behind", "match on both sides", "no match", "delimiter on the last byte in front",
                "delimiter on the first byte behind")


def mixed(needle):
    """the needle with every other letter in upper case (at least one, so that it is no copy of the needle)"""
    out, k = bytearray(needle), 0
    for j, c in enumerate(needle):
        if 0x61 <= c <= 0x7A:
            if k % 2 == 0:
                out[j] = c ^ 0x20
            k += 1
    assert bytes(out) != bytes(needle), "the needle holds no lower-case letter"
    return bytes(out)


class Grid:
    """`ntiles` tiles of `tile` bytes, `tpw` contiguous tiles per workgroup, over a view of `length` bytes; tile k (k >= 1) begins at
    byte k * tile + shift, tile 0 at byte 0 (the bytes in front of the filter stream are scanned apart, and counted to it here)"""
    def __init__(self, length, tile, tpw, ntiles, shift=0):
        self.length, self.tile, self.tpw, self.ntiles, self.shift = length, tile, tpw, ntiles, shift
        self.nwg = -(-ntiles // tpw)
        assert 0 <= shift < tile and self.border(ntiles - 1) < length

    def border(self, k):
        """the first byte of tile k"""
        return k * self.tile + self.shift if k > 0 else 0

    def start(self, w):
        """the first byte of workgroup w"""
        return self.border(w * self.tpw)

    def tile_of(self, at):
        return np.minimum(np.maximum(np.asarray(at, dtype=np.int64) - self.shift, 0) // self.tile, self.ntiles - 1)

    def workgroup_of(self, at):
        return self.tile_of(at) // self.tpw


def _reach(needle):
    """(n, g): scenes around a border stay within 2 g + n bytes of it; a match meant for one side is g bytes or more away"""
    return len(needle), len(needle) + 3


def tile_border_scenes(kind, sub, T, E, needle):
    """one scene kind (an index into KINDS) around the inner tile border T of a two-tile workgroup that ends at E (the next one's
    first byte); `sub` counts the kind's uses and walks its variants"""
    n, g = _reach(needle)
    N = needle
    if kind == 9:
        kind, sub, N = (0, 3, 7, 8)[sub % 4], sub // 4, mixed(needle)
    if kind == 0:
        return [(T - g - n, NL + N), (T + g, NL)]
    if kind == 1:
        return [(T - 1, NL + N + b" " + NL)]
    if kind == 2:
        return [(T - g - n, NL + N), (T, NL + N + NL)]
    if kind == 3:
        j = 1 + sub % (n - 1)                               # bytes of the occurrence in front of T
        return [(T - j - 1, NL + N + NL)]
    if kind == 4:
        return [(E - g - n, NL + N), (E + 2, NL)]
    if kind == 5:
        return [(E - g, NL), (E + 1, N + NL)]
    if kind == 6:
        return [(T - g, NL + b"kk"), (T + g, NL)]
    r = (b"k", b" ", NL)[sub % 3]
    if kind == 7:
        return [(T - n - 1, NL + N + r + NL)]               # the occurrence is [T - n, T), r is the byte at T
    assert kind == 8
    return [(T - 2, NL + r + N + NL)]                       # r is the byte at T - 1, the occurrence begins at T


def two_tile_scenes(grid, needle, workgroups, long_line=None, notes=None):
    """Scenes for a grid of two tiles per workgroup whose last workgroup has one: in every workgroup of `workgroups` a line that
    matches under every `how` in each tile, and around its inner tile border one of KINDS, cycling; a copy at offset 0 when
    workgroup 0 is chosen; an unterminated matching last line flush with the view's end when the last one is.  long_line = (w0, w1,
    wm): one line from workgroup w0 to workgroup w1 whose only match is in the second tile of workgroup wm; none of w0 - 1 .. w1 may
    be chosen.  notes (a dict) takes workgroup -> what was planted there."""
    assert grid.tpw == 2 and grid.ntiles % 2 == 1 and len(needle) >= 2
    n, g = _reach(needle)
    lead = n + g + 2                                        # a workgroup's first bytes belong to the scenes of the one in front
    assert grid.tile // 3 >= lead + 1 and grid.tile // 3 + grid.tile // 4 + n + 3 <= grid.tile - max(2 * g + n, 8) - 1, "tile too small"
    notes = {} if notes is None else notes
    scenes, uses = [], {}
    wgs = sorted(set(int(w) for w in workgroups))
    assert wgs and 0 <= wgs[0] and wgs[-1] < grid.nwg
    if long_line:
        w0, w1, wm = long_line
        assert w0 < wm < w1 < grid.nwg - 1 and not [w for w in wgs if w0 - 1 <= w <= w1]
        scenes += [(grid.start(w0) + lead, NL), (grid.border(2 * wm + 1) + grid.tile // 2, needle), (grid.start(w1) + lead, NL)]
        notes[w0], notes[wm], notes[w1] = "the long line opens", "the long line's only match, second tile", "the long line closes"
    cycle = 0
    for w in wgs:
        S, T, E = grid.start(w), grid.border(2 * w + 1), grid.start(w + 1)
        jitter = (w * 37) % (grid.tile // 4)
        left = (b"", b" ", b"k")[w % 3]                     # the first tile's line: a whole line, a word, or neither
        scenes.append((max(S, 0) + grid.tile // 3 + jitter - len(left), NL + left + needle + NL))
        if w == 0:
            scenes.append((0, needle + b" "))               # p == 0: the left neighbour is absent
        if w == grid.nwg - 1:
            scenes.append((grid.length - n - 1, NL + needle))
            notes[w] = "the last workgroup: one tile, an unterminated matching last line"
            continue
        kind = cycle % len(KINDS)
        sub = uses.get(kind, 0)
        uses[kind] = sub + 1
        cycle += 1
        scenes.append((T + grid.tile // 3 + jitter, NL + needle + NL))
        scenes += tile_border_scenes(kind, sub, T, E, needle)
        notes[w] = "kind %d.%d: %s" % (kind, sub, KINDS[kind])
    notes["uses"] = uses                                    # kind -> how many workgroups hold it
    return _checked(scenes, grid.length)


def border_scenes(kind, X, needle):
    """one of BORDER_KINDS: a line across the byte border X (a border between two parts, two chunks of parts or two runs of chunks)
    with its match in front of X, behind it, on both sides or on neither; or a delimiter on the byte next to X"""
    n, g = _reach(needle)
    if kind == 0:
        return [(X - g - n, NL + needle), (X + g, NL)]
    if kind == 1:
        return [(X - g, NL), (X + g, needle + NL)]
    if kind == 2:
        return [(X - g - n, NL + needle), (X + g, needle + NL)]
    if kind == 3:
        return [(X - g, NL + b"kk"), (X + g, NL)]
    if kind == 4:
        return [(X - g - n - 1, NL + needle), (X - 1, NL + needle + NL)]
    assert kind == 5
    return [(X - g - n, NL + needle), (X, NL + needle + NL)]


def background_scenes(grid, needle, workgroups):
    """a matching and a not matching line in the middle of the first tile of each of `workgroups`, so that the states carried past
    the borders under test are not the empty ones; in turn the copy is a whole line, in mixed case, and glued to a word byte"""
    out = []
    for k, w in enumerate(workgroups):
        at = grid.start(w) + grid.tile // 3 + (w * 37) % (grid.tile // 4)
        out.append((at, NL + (needle, mixed(needle), b"k" + needle)[k % 3] + NL + b"kk" + NL))
    return out


def _checked(scenes, length):
    """sorted, inside the view, not overlapping (touching is fine)"""
    scenes = sorted((int(o), bytes(b)) for o, b in scenes)
    at = 0
    for o, b in scenes:
        assert o >= at and len(b) > 0 and o + len(b) <= length, ("scenes overlap or leave the view", o, b, at, length)
        at = o + len(b)
    return scenes


def checked(scenes, length):
    return _checked(scenes, length)


def write_scenes(array, scenes):
    """the scenes into a numpy array that holds the filler"""
    for o, b in scenes:
        array[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return array


def _groups(scenes, n):
    """scenes closer to each other than 2 n + 2 bytes, as (offset, text) with the filler between them written out"""
    fill = bytes([FILLER])
    out = []
    for o, b in scenes:
        if out and o - (out[-1][0] + len(out[-1][1])) <= 2 * n + 2:
            p, t = out[-1]
            out[-1] = (p, t + fill * (o - p - len(t)) + b)
        else:
            out.append((o, bytearray(b)))
    return out


def sparse_lines(scenes, length, needle, delim, how, inverted):
    """(begin, end, number) int64 arrays of the lines that a view of `length` filler bytes with `scenes` written into it selects:
    the lines that hold an occurrence of `needle` under `how` - ignoring case, kept as a whole word or a whole line - or, inverted,
    the other lines.  A trailing empty piece is no line, an unterminated last piece is one."""
    assert how in HOWS
    scenes = _checked(scenes, length)
    needle = bytes(needle)
    n, nocase, bound = len(needle), how.endswith("i"), how[:1] if how[:1] in ("w", "x") else ""
    nd = needle.lower() if nocase else needle
    assert n >= 1 and delim != FILLER and FILLER not in needle.lower() and FILLER not in needle.upper() and FILLER not in _WORD
    dpos = np.array([o + j for o, b in scenes for j, c in enumerate(b) if c == delim], dtype=np.int64)
    begins = np.concatenate((np.zeros(1, dtype=np.int64), dpos + 1))
    ends = np.concatenate((dpos, np.full(1, length, dtype=np.int64)))
    if begins[-1] == length:
        begins, ends = begins[:-1], ends[:-1]
    kept = []
    if delim not in nd and n <= length:
        fill = bytes([FILLER])
        for o, t in _groups(scenes, n):
            a, z = max(0, o - n), min(length, o + len(t) + n)
            text = fill * (o - a) + bytes(t) + fill * (z - o - len(t))
            fold = text.lower() if nocase else text
            p = fold.find(nd)
            while p >= 0:
                # a neighbour is absent only where the text ends with the view (the filler is no needle byte)
                assert (p > 0 or a == 0) and (p + n < len(text) or z == length)
                ok = True
                for at in (p - 1, p + n):
                    if bound and 0 <= at < len(text):
                        ok &= text[at] == delim or (bound == "w" and text[at] not in _WORD)
                if ok:
                    kept.append(a + p)
                p = fold.find(nd, p + 1)
    kept = np.array(sorted(set(kept)), dtype=np.int64)
    first = np.searchsorted(dpos, kept, side="left")
    inside = np.searchsorted(dpos, kept + n - 1, side="right") == first        # (folded, a delimiter 'A' can look like a needle byte)
    hit = np.zeros(begins.size, dtype=bool)
    hit[np.unique(first[inside])] = True
    pick = ~hit if inverted else hit
    return begins[pick], ends[pick], np.arange(1, begins.size + 1, dtype=np.int64)[pick]

"""Scenes on a haystack of one filler byte for the five libraries that share needleset_launch.hpp's geometry - needleset, setmatches,
masked, classes, runs - and ONE reference for all of them, worked out from the scenes alone (a helper of tests/test_gpu_set_grids.py
and tests/test_set_sparse_cpu.py, not a test module).

A SCENE is a short byte string at a known offset; everything between the scenes is FILLER, which is no delimiter, no word byte, no
byte of any needle, no member of any class and accepted by no fixed position of a masked pattern.  A KIT names what one pattern makes
of bytes: `hits` (each holds an occurrence, or is one selected run), `straddle` (what is laid across a border: a hit, and for runs a run that
the bounds reject) and `margin` (the pattern length; `look` bytes for runs).  The builders place the kit's bytes where the line
bookkeeping and the ranks carry state - the border between two parts, between two chunks of parts, a chunk without a delimiter, the
view's end - for a part size that is a parameter, so that the same kinds fit into a few KiB at 64 bytes per part and into hundreds of
MiB at 128 KiB.

The REFERENCE never sees the haystack.  `sparse_spans` groups neighbouring scenes, widens each group by `margin` filler bytes,
materialises that group alone and hands it to the suite's dense rule, passed in as a callable `array -> (start, end, tag)`;
`sparse_lines` takes delimiters, line numbers, begins and ends from the scene list and selects the lines that hold a span without a
delimiter inside (runs are cut at delimiters by their rule); `sparse_gaps` is the one pattern whose set holds the FILLER, `[^\\n]{k,}`:
its runs are the gaps between delimiters.  tests/test_set_sparse_cpu.py holds all three against the dense rules on real arrays."""
import bisect

import numpy as np

FILLER = 0x2E                                   # '.'
NL = b"\n"
DELIM = 10
WG = 131072                                     # bytes of the aligned stream per workgroup ("part"): kSetTiles tiles of 16 KiB
CHUNK = 256                                     # parts per workgroup of lines_chunk_kernel
THREADS = 1024                                  # threads of prefix_kernel and of lines_combine_kernel
GAP = 2                                         # filler bytes between a scene and the border it is meant to stay off
KINDS = ("a: match in front of the border, the line closes behind it", "b: delimiter on the last byte in front, match begins on the border",
         "c: delimiter on the border, match in front", "d: an occurrence or run straddles the border",
         "e: an occurrence ends on the last byte in front or begins on the border; the outside neighbour a word byte, a blank, the delimiter",
         "f: a line without a match across the border")
LONG_LINE = ("the only match in the first chunk", "the only match in the middle chunk", "no match")


class Parts:
    """A view of `length` bytes whose first byte lies `mis` bytes behind a part border: part k (k >= 1) begins at view offset
    k * part - mis, part 0 at offset 0; `chunk` parts make a chunk of lines_chunk_kernel, thread t of the prefix owns `per` parts."""
    def __init__(self, length, part=WG, mis=0, chunk=CHUNK, threads=THREADS):
        assert length > 0 and 0 <= mis < part
        self.length, self.part, self.mis, self.chunk = length, part, mis, chunk
        self.parts = -(-(mis + length) // part)
        self.chunks = -(-self.parts // chunk)
        self.per = -(-self.parts // threads)

    def border(self, k):
        """the first byte of part k"""
        return k * self.part - self.mis if k > 0 else 0

    def part_of(self, at):
        return (np.asarray(at, dtype=np.int64) + self.mis) // self.part

    def __repr__(self):
        return "parts %d, chunks %d, per %d (mis %d)" % (self.parts, self.chunks, self.per, self.mis)


class Kit:
    """what one pattern makes of bytes: each of `hits` holds an occurrence (or is a selected run) and no filler, `straddle` goes
    across borders in kind d, `margin` filler bytes on both sides of a group of scenes are enough for the dense rule to see every
    occurrence that touches the group"""
    def __init__(self, name, hits, margin, straddle=None):
        self.name, self.hits, self.margin = name, [bytes(h) for h in hits], int(margin)
        self.straddle = [bytes(s) for s in (straddle or self.hits[:1])]
        assert all(len(s) >= 2 for s in self.straddle) and all(FILLER not in h and h for h in self.hits)
        self.reach = max(len(x) for x in self.hits + self.straddle) + GAP + 2     # scenes of a border stay this close to it

    def hit(self, k):
        return self.hits[k % len(self.hits)]

    def variants(self, kind):
        return {3: 3 * len(self.straddle), 4: 6}.get(kind, 1)


def border_scenes(kind, sub, B, kit):
    """one of KINDS around the border B (the first byte of a part); `sub` walks the kind's variants and the kit's hits"""
    h = kit.hit(sub)
    n = len(h)
    if kind == 0:
        return [(B - GAP - n - 1, NL + h), (B + GAP, NL)]
    if kind == 1:
        return [(B - 1, NL + h + NL)]
    if kind == 2:
        return [(B - GAP - n - 1, NL + h), (B, NL)]
    if kind == 3:
        s = kit.straddle[sub % len(kit.straddle)]
        j = (1, len(s) // 2, len(s) - 1)[(sub // len(kit.straddle)) % 3]     # bytes in front of B
        return [(B - j - 1, NL + s + NL)]
    if kind == 4:
        r = (b"k", b" ", NL)[(sub // 2) % 3]
        if sub % 2 == 0:
            return [(B - n - 1, NL + h + r + NL)]                # the occurrence is [B - n, B), r is the byte at B
        return [(B - 2, NL + r + h + NL)]                        # r is the byte at B - 1, the occurrence begins at B
    assert kind == 5
    return [(B - GAP, NL), (B + GAP, NL)]


def long_line_scenes(pt, kit, w_open, w_close, variant):
    """kind g: one line from the middle of part w_open to the middle of part w_close, two chunks on, the chunk between without a
    delimiter; its only match behind the opening delimiter, in the middle chunk, or nowhere (LONG_LINE)"""
    c = w_open // pt.chunk
    assert w_close // pt.chunk == c + 2 and w_close < pt.parts - 1
    half = pt.part // 2
    out = [(pt.border(w_open) + half, NL), (pt.border(w_close) + half, NL)]
    if variant == 0:
        out.append((pt.border(w_open) + half + GAP + 1, kit.hit(0)))
    elif variant == 1:
        out.append((pt.border((c + 1) * pt.chunk + pt.chunk // 2) + half, kit.hit(1)))
    return out


def grid_scenes(pt, kit, rot, borders, long_line=None, flush=(), thin=1, notes=None):
    """The scenes of one view: at border k = borders[j] kind (j + rot) % 6 with variant j (so that six rotations show every kind at
    every border, and six borders every variant); kind g (long_line = (w_open, w_close), variant rot % 3); kind h, an unterminated
    matching last line flush with the view's end and with every other end of `flush` (the ends of shorter views of the same bytes,
    cut out with `view_scenes`); a hit on the view's first byte; and kind i, the background: every `thin`-th part w outside the long
    line holds 1 + (7 w mod 5) matching one-line scenes at offsets that vary with w, wherever the scenes above leave room.
    notes (a dict) takes border -> (kind, variant)."""
    notes = {} if notes is None else notes
    first = []
    for j, k in enumerate(borders):
        assert 1 <= k < pt.parts and not (long_line and long_line[0] < k <= long_line[1]), k
        kind = (j + rot) % len(KINDS)
        first += border_scenes(kind, j, pt.border(k), kit)
        notes[k] = (kind, j % kit.variants(kind))
    if long_line:
        first += long_line_scenes(pt, kit, long_line[0], long_line[1], rot % 3)
        notes["long line"] = rot % 3
    for end in tuple(flush) + (pt.length,):
        first.append((end - len(kit.hit(rot)) - 1, NL + kit.hit(rot)))
    first.append((0, kit.hit(rot + 1) + NL))
    first = checked(first, pt.length)
    taken = [(o - 1, o + len(b) + 1) for o, b in first]         # background scenes keep a byte of filler off them
    starts = [t[0] for t in taken]
    room = pt.part - 2 * kit.reach
    slot = room // 5
    longest = max(len(h) for h in kit.hits) + 2
    assert slot >= longest, ("the part is too small for the kit", pt.part, kit.name)
    back = []
    for w in range(0, pt.parts, thin):
        if long_line and long_line[0] <= w <= long_line[1]:
            continue
        for j in range(1 + (7 * w) % 5):
            h = kit.hit(5 * w + j)
            at = pt.border(w) + kit.reach + slot * j + (w * 37) % (slot - longest + 1)
            k = bisect.bisect_right(starts, at + len(h) + 2) - 1
            if at + len(h) + 2 > pt.length - kit.reach or (k >= 0 and taken[k][1] > at) or (k >= 1 and taken[k - 1][1] > at):
                continue
            back.append((at, NL + h + NL))
    notes["background"] = len(back)
    return checked(first + back, pt.length)


def checked(scenes, length):
    """sorted, inside the view, not overlapping (touching is fine)"""
    scenes = sorted((int(o), bytes(b)) for o, b in scenes)
    at = 0
    for o, b in scenes:
        assert o >= at and len(b) > 0 and o + len(b) <= length, ("scenes overlap or leave the view", o, b, at, length)
        at = o + len(b)
    return scenes


def view_scenes(scenes, lo, hi):
    """the scenes of the view [lo, hi) of the same bytes, in the view's offsets; a scene that an end of the view cuts is cut"""
    out = []
    for o, b in scenes:
        a, z = max(o, lo), min(o + len(b), hi)
        if a < z:
            out.append((a - lo, b[a - o:z - o]))
    return out


def write_scenes(array, scenes):
    """the scenes into a numpy array that holds the filler"""
    for o, b in scenes:
        array[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return array


def _groups(scenes, margin):
    """scenes closer to each other than 2 margin + 2 bytes, as (offset, text) with the filler between them written out"""
    fill = bytes([FILLER])
    out = []
    for o, b in scenes:
        if out and o - (out[-1][0] + len(out[-1][1])) <= 2 * margin + 2:
            p, t = out[-1]
            t += fill * (o - p - len(t)) + b
        else:
            out.append((o, bytearray(b)))
    return out


def sparse_spans(scenes, length, margin, rule, cache=None):
    """(start, end, tag) int64 arrays, ordered by (start, tag), of what `rule` finds in a view of `length` filler bytes with `scenes`
    written into it.  rule(array) -> (start, end, tag) is a dense rule of the suite on a small array; it runs once per distinct
    group text (`cache`, a dict, carries the results from one call to the next)."""
    scenes = checked(scenes, length)
    cache = {} if cache is None else cache
    fill = bytes([FILLER])
    parts = []
    for o, t in _groups(scenes, margin):
        a, z = max(0, o - margin), min(length, o + len(t) + margin)
        text = fill * (o - a) + bytes(t) + fill * (z - o - len(t))
        if text not in cache:
            s, e, g = (np.asarray(x, dtype=np.int64) for x in rule(np.frombuffer(text, dtype=np.uint8)))
            # every span touches a scene byte, so none reaches the filler that the group does not hold (absent only at the view's ends)
            assert s.size == e.size == g.size and (e > s).all()
            cache[text] = (s, e, g)
        s, e, g = cache[text]
        assert ((s > 0) | (a == 0)).all() and ((e < len(text)) | (z == length)).all()
        parts.append((s + a, e + a, g))
    if not parts:
        return tuple(np.zeros(0, dtype=np.int64) for _ in range(3))
    s, e, g = (np.concatenate([p[k] for p in parts]) for k in range(3))
    order = np.lexsort((g, s))
    return s[order], e[order], g[order]


def delimiters(scenes, delim=DELIM):
    return np.array([o + j for o, b in scenes for j, c in enumerate(b) if c == delim], dtype=np.int64)


def sparse_gaps(scenes, length, delim, lo, hi=None):
    """(start, end, tag) of the runs of a set that holds every byte but `delim` - the FILLER too: the non-empty gaps between
    delimiters whose length lies in [lo, hi]"""
    dpos = delimiters(checked(scenes, length), delim)
    b = np.concatenate((np.zeros(1, dtype=np.int64), dpos + 1))
    e = np.concatenate((dpos, np.full(1, length, dtype=np.int64)))
    keep = (e - b >= max(lo, 1)) & ((e - b <= hi) if hi else True)
    return b[keep], e[keep], np.zeros(int(keep.sum()), dtype=np.int64)


def sparse_lines(scenes, length, spans, delim=DELIM, inverted=False):
    """(begin, end, number) int64 arrays of the lines that hold one of `spans` = (start, end, ...) with no delimiter inside it - or,
    inverted, of the other lines.  A trailing empty piece is no line, an unterminated last piece is one."""
    dpos = delimiters(checked(scenes, length), delim)
    begins = np.concatenate((np.zeros(1, dtype=np.int64), dpos + 1))
    ends = np.concatenate((dpos, np.full(1, length, dtype=np.int64)))
    if begins[-1] == length:
        begins, ends = begins[:-1], ends[:-1]
    s, e = np.asarray(spans[0], dtype=np.int64), np.asarray(spans[1], dtype=np.int64)
    first = np.searchsorted(dpos, s, side="left")
    inside = np.searchsorted(dpos, e - 1, side="right") == first
    hit = np.zeros(begins.size, dtype=bool)
    hit[np.unique(first[inside])] = True
    pick = ~hit if inverted else hit
    return begins[pick], ends[pick], np.arange(1, begins.size + 1, dtype=np.int64)[pick]


# ---- the two shapes of tests/test_gpu_set_grids.py ----------------------------------------------------------------------------------
END_A = 258 * WG - 4099                         # shape A ends here in the buffer's offsets, at either misalignment: 258 parts
LEN_B = 1536 * WG + 40013                       # shape B: 1,537 parts, the last chunk of one part
BORDERS_B = (256, 257, 512, 1280, 1536, 1535, 1, 255, 1281, 700)
LONG_B = (2 * CHUNK + 200, 4 * CHUNK + 50)      # kind g: opens in chunk 2, closes in chunk 4
ROTATIONS = len(KINDS)


def shape_a(mis):
    return Parts(END_A - mis, WG, mis)


def shape_b():
    return Parts(LEN_B, WG, 0)


def buffer_scenes(kit, rot, thin=1, notes=None):
    """the scenes of shape B's buffer; shape A's are view_scenes(.., mis, END_A)"""
    return grid_scenes(shape_b(), kit, rot, BORDERS_B, LONG_B, flush=(END_A,), thin=thin, notes=notes)

#!/usr/bin/env python3
"""./grep_hip.py [-i] [-w | -x] [-v] <needle> <file> [--count | --offsets | --count-lines | --lines] - the reference's examples/grep.rs:42-56 with the
"hip" backend: map the file, build one searcher, one search_in, print the boolean.
  --count        the number of (overlapping) OCCURRENCES, not lines (libsliceslice_hip_matches.so, ss_count_device)
  --offsets      grep -b -o style: one byte offset per occurrence, ascending (ss_find_all_device)
  --count-lines  grep -c: the number of LINES that contain the needle (libsliceslice_hip_lines.so, ss_count_lines_device)
  --lines        grep -n: `number:line` for every line that contains the needle (ss_find_lines_device; only the records and the
                 bytes of those lines travel to the host)
  -i, --ignore-case  with one of the four switches above: ASCII letters match in either case, every other byte exactly (grep -i
                 in the C locale; libsliceslice_hip_nocase.so, the ss_*_nocase_device calls).  The line delimiter is not folded.
  -w, --word-regexp  with one of the four switches: only occurrences that stand as whole words - both neighbour bytes absent, the
                 line's end (line outputs) or outside [0-9A-Za-z_] (grep -w in the C locale; libsliceslice_hip_bounded.so, the
                 ss_*_bounded_device calls).  Combines with -i.  The empty needle is refused.
  -x, --line-regexp  with --count-lines or --lines: only lines that ARE the needle (grep -x).  Combines with -i, not with -w; with
                 the occurrence outputs it is an error.
  -v, --invert-match  with --count-lines or --lines: the lines that do NOT match (grep -v; libsliceslice_hip_inverted.so, the
                 ss_*_lines_inverted_device calls).  Combines with -i, -w and -x.  There is no inverted occurrence form -
                 occurrences have no complement - so --count and --offsets refuse it, and so do several patterns (-e / -f).
  -A NUM, -B NUM, -C NUM (--after-context, --before-context, --context; also -ANUM and --context=NUM)  with --lines only: NUM
                 lines behind / in front of / around every selected line as well, each line once - `number:line` for the selected
                 lines, `number-line` for the context lines and `--` between groups that are not adjacent, byte for byte what
                 `LC_ALL=C grep -F -n` prints (libsliceslice_hip_context.so, ss_find_lines_context_device).  Combines with -i, -w,
                 -x and -v.  The counting outputs, the plain search and several patterns (-e / -f) refuse them.
./grep_hip.py --count (-e <pattern>)... [-f <patterns file>] <file> - several patterns (-e repeated; -f: one per line): one count
per pattern and line, in the order given, from ONE call (libsliceslice_hip_matches_batched.so, ss_count_batched).  The batched
library has no case-folding and no whole-word form: -i, -w and -x with -e / -f and --count are refused.
./grep_hip.py (--count-lines | --lines) [-i] [-w | -x] [-v] [-A NUM] [-B NUM] [-C NUM] (-e <pattern>)... [-f <patterns file>] <file> -
the LINES that match ANY of the patterns (grep -e A -e B, grep -f FILE; -e may also stand once): --count-lines prints their
number, --lines prints `number:line` for each - and, with -A / -B / -C (--lines only), the context lines as `number-line` and `--`
between groups - byte for byte what `LC_ALL=C grep -F -c` / `LC_ALL=C grep -F -n` print (libsliceslice_hip_anyof.so,
ss_count_lines_anyof_device / ss_find_lines_anyof_device: one searcher per pattern, the flags apply to every pattern; -v selects
the lines that match none).
./grep_hip.py --one-pass (--count-lines | --lines) ... (-e <pattern>)... [-f <patterns file>] <file> - the same output, byte for byte,
by ONE scan of the file for all patterns instead of one per pattern (libsliceslice_hip_needleset.so, ss_count_lines_set_device /
ss_find_lines_set_device: the patterns are compiled into a set once).  --one-pass goes with -e / -f and --count-lines or --lines
only; without it nothing changes.
./grep_hip.py --frequencies [-i] [-w] (-e <pattern>)... [-f <patterns file>] <file> - a word-frequency table: one count of
(overlapping) OCCURRENCES per pattern and line, in the order given, from ONE scan of the file for all patterns
(libsliceslice_hip_setmatches.so, ss_count_set_device: the patterns are compiled into a set once, and the counts per distinct
pattern are gathered back into the order given).  Without -i / -w the output is byte for byte what --count -e ... prints.  -x, -v
and -A / -B / -C are refused: occurrences know no line, have no complement and no context; so is the empty pattern.
./grep_hip.py -o (--count | --offsets) [-i] [-w] <needle> <file> - the NON-OVERLAPPING occurrences, taken greedily from the left
(-o, --only-matching; libsliceslice_hip_disjoint.so, ss_count_disjoint_device / ss_find_all_disjoint_device): --count prints their
number (bytes.count), --offsets prints `offset:match` for each, byte for byte what grep -o -b -F prints (with -i the match is the
file's own bytes).  Without -o, --count and --offsets stay what they were: every overlapping occurrence.
./grep_hip.py --replace <text> [-i] [-w] <needle> <file> - the file with every non-overlapping occurrence replaced by <text>, to
stdout (sed 's/needle/text/g' for a fixed string, bytes.replace; ss_replace_device: the substituted bytes are made on the device).
Both refuse -x, -v, -A / -B / -C, --count-lines, --lines, --frequencies and -e / -f: the non-overlapping selection is about the
occurrences of one needle; --replace refuses the empty needle.
./grep_hip.py -o (--count | --offsets) [-i] [-w] (-e <needle>)... [-f <needles file>] <file> - -o with -e / -f: the LEFTMOST-LONGEST,
non-overlapping occurrences of a SET of needles - at each offset the longest needle, taken greedily from the left, the word test
first - --count their number and --offsets `offset:match` for each, byte for byte what LC_ALL=C grep -o -b -F prints for those
patterns (libsliceslice_hip_leftmost.so, ss_count_leftmost_set_device / ss_find_all_leftmost_set_device: the selection is made on the
device).
./grep_hip.py --replace-map <map file> [-i] [-w] <file> - the file with each of those occurrences replaced by its needle's own text, to
stdout; the map file holds one `needle<TAB>text` pair per line (re.sub over an alternation of literals with a replacement per
literal; ss_replace_set_device).  Both refuse -x, -v, -A / -B / -C, --count-lines, --lines, --frequencies, --one-pass, --device-output
and --replace, and the empty needle.
./grep_hip.py --device-output --lines [-i] [-w | -x] [-v] [-A NUM] [-B NUM] [-C NUM] [--one-pass] (<needle> | (-e <pattern>)... [-f
<patterns file>]) <file> - what --lines prints, byte for byte, with the text made ON THE DEVICE: the lines are gathered, numbered
(`number:` / `number-`), terminated and separated by `--` there, and the finished text comes to the host in one copy
(libsliceslice_hip_output.so: ss_grep_lines_device for one needle, ss_find_lines_anyof_device or ss_find_lines_set_device followed by
ss_format_lines_device for several).  --device-output goes with --lines only; without it nothing changes.
./grep_hip.py --hex '<pattern>' (--count | --offsets | --count-lines | --lines) [--device-output] <file> - a byte pattern with
wildcards and per-byte masks in ONE pass (libsliceslice_hip_masked.so, include/sliceslice_hip_masked.h): tokens of two characters,
each a hex digit or `?`, such as '48 8b ?? 4?'.  --count prints the number of (overlapping) occurrences, --offsets one offset per
line, --count-lines the number of lines that hold an occurrence wholly inside them and --lines those lines as `number:line`;
with --device-output the text of --lines is made on the device (ss_format_lines_device).  Every other flag is refused.
./grep_hip.py --classes '<pattern>' [-i] (--count | --offsets | --count-lines | --lines) [--device-output] <file> - a fixed-length
pattern of byte classes in ONE pass (libsliceslice_hip_classes.so, include/sliceslice_hip_classes.h, which has the pattern language:
a strict subset of Python `re` byte patterns under re.DOTALL), such as '[0-9A-F]{4}H', '\\d\\d:\\d\\d' or '[^a-z]the[^a-z]'.  The four modes
and --device-output are those of --hex; -i is re.I.  Every other flag is refused, and a pattern the language refuses is reported
with its column.
./grep_hip.py --runs '<pattern>' [-i] (--count | --offsets | -o | --count-lines | --lines) [--device-output] <file> - the maximal runs
of ONE byte class in ONE pass (libsliceslice_hip_runs.so, include/sliceslice_hip_runs.h): one item of the classes language and one of
+ {k} {k,} {k,m}, such as '\\w+', '[0-9]{3,}' or '[A-Z]{2,5}'; a run that is too long is not selected and no run is chopped.  --count
prints the number of selected runs, --offsets `begin:end` per run, -o the runs themselves, one per line (ss.gather_ranges: what
`grep -o -E` prints when there is no maximum), --count-lines and --lines the lines that hold a selected run (--device-output as
above); -i is re.I.
./grep_hip.py --runs '<pattern>' [-i] --replace <text> [--per-line] <file> - the file with every selected run replaced by <text>, on
stdout (libsliceslice_hip_rewrite.so, include/sliceslice_hip_rewrite.h: `sed -E 's/<pattern>/<text>/g'`, `tr -d`, `tr -s`); an empty
<text> deletes; --per-line passes the delimiter `\n`, which is then never a member, so that '\\s+' works line by line as in sed.  It
is not combined with the five listing modes.
./grep_hip.py --fields <list> -d <sep> [--merge] [-s] [--device-output] <file> - fields first .. last of every line, one line of output
per record (libsliceslice_hip_fields.so, include/sliceslice_hip_fields.h: `cut -d, -f3`, `awk '{print $2}'`).  <list> is cut's single
range K, K-, K-M or -M (a comma list is refused: one call per range); <sep> is one character or one item of the classes language
such as '[ \\t]'; --merge takes runs of separators as one and ignores leading and trailing ones, as awk does.  -s prints nothing for a
line that lacks field `first`; without it such a line gives an empty line, so that the output has one line per input line.  With
--device-output the text is gathered on the device (ss.gather_ranges) and comes to the host in one copy.  THE ONE DIFFERENCE FROM
cut: a line without any separator is treated as a line with one field - cut prints such a line whole, whatever the list says.
./grep_hip.py --runs '<pattern>' --uniq-count [-i] [--top <k>] [--device-output] <file> - `count<TAB>token` per DISTINCT selected run, in
first-occurrence order (libsliceslice_hip_groups.so, include/sliceslice_hip_groups.h: `grep -oE '<pattern>' | sort | uniq -c` before
the sort, a collections.Counter filled in input order).  --top <k> prints the k most frequent, most frequent first, ties in
first-occurrence order.  -i folds ASCII letters before tokens are compared; the token printed is the first occurrence as it stands.
With --device-output the tokens are gathered on the device (ss.gather_ranges) and come to the host in one copy.
./grep_hip.py --lines-uniq-count [-i] [--top <k>] [--device-output] <file> - the same for whole lines: sorted, this is `sort | uniq -c`.
./grep_hip.py --uniq [-i] [--device-output] <file> - every distinct line once, in input order (`awk '!seen[$0]++'`).
./grep_hip.py --help prints this text."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sliceslice_rs_amd as ss  # noqa: E402


def count_patterns(patterns, filename):
    """One count_batched call: every pattern against the whole file (aliased haystack ranges)."""
    import numpy as np
    import torch
    data = np.fromfile(filename, dtype=np.uint8)
    blob = np.frombuffer(b"".join(patterns) + b"\x00", dtype=np.uint8).copy()
    cuts = np.cumsum([0] + [len(p) for p in patterns]).astype(np.int64)
    with ss.matches_batched_build():
        hb = torch.zeros(len(patterns), dtype=torch.int64, device="cuda")
        he = torch.full((len(patterns),), data.size, dtype=torch.int64, device="cuda")
        counts = ss.count_batched(torch.from_numpy(data).cuda(), None, torch.from_numpy(blob).cuda(), torch.from_numpy(cuts).cuda(),
                                  hay_ranges=(hb, he))
        return counts.cpu().tolist()


def matching_lines(searcher, data, ignore_case=False, invert=False, **bound):
    """[(number, line bytes)] of the lines that contain the needle (invert: of those that do not): the records, then only those byte
    ranges, come to the host."""
    import torch
    hay = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if data else torch.empty(0, dtype=torch.uint8, device="cuda")
    begin, end, number = (searcher.find_lines_inverted if invert else searcher.find_lines)(hay, ignore_case=ignore_case, **bound)
    if begin.numel() == 0:
        return []
    # gather the matching lines' bytes on the device: one copy of sum(end - begin) bytes instead of the whole file
    length = end - begin
    start = torch.cumsum(length, 0) - length
    idx = torch.repeat_interleave(begin - start, length) + torch.arange(int(length.sum()), device=hay.device)
    packed = hay[idx].cpu().numpy().tobytes()
    out, at = [], 0
    for n, ln in zip(number.cpu().tolist(), length.cpu().tolist()):
        out.append((n, packed[at:at + ln]))
        at += ln
    return out


_CONTEXT_FLAGS = {"-A": "after", "--after-context": "after", "-B": "before", "--before-context": "before", "-C": "both", "--context": "both"}


def context_amount(flag, text):
    if not (text.isascii() and text.isdigit()):
        raise SystemExit("./grep_hip.py: %s takes a non-negative integer (a number of context lines), got %r" % (flag, text))
    return int(text)


def context_lines(searcher, data, before, after, ignore_case=False, invert=False, **bound):
    """grep's output for -B before -A after -n, as bytes: like matching_lines, the records first, then only the bytes of the
    printed lines, gathered on the device."""
    import torch
    hay = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if data else torch.empty(0, dtype=torch.uint8, device="cuda")
    if isinstance(searcher, ss.NeedleSet):                      # --one-pass: the fold is the set's
        find = lambda *a, ignore_case=False, **kw: searcher.find_lines(*a, **kw)         # noqa: E731
    elif isinstance(searcher, list):                            # several patterns: the lines that match any of them
        find = lambda *a, **kw: ss.find_lines_anyof(searcher, *a, **kw)                  # noqa: E731
    else:
        find = searcher.find_lines_context
    begin, end, number, kind = find(hay, min(before, 2 ** 64 - 1), min(after, 2 ** 64 - 1), ignore_case=ignore_case, invert=invert, **bound)
    if begin.numel() == 0:
        return b""
    length = end - begin
    start = torch.cumsum(length, 0) - length
    idx = torch.repeat_interleave(begin - start, length) + torch.arange(int(length.sum()), device=hay.device)
    packed = hay[idx].cpu().numpy().tobytes()
    out, at, last = [], 0, None
    for n, ln, k in zip(number.cpu().tolist(), length.cpu().tolist(), kind.cpu().tolist()):
        if last is not None and n > last + 1:
            out.append(b"--\n")
        out.append(b"%d%s%s\n" % (n, b":" if k else b"-", packed[at:at + ln]))
        at += ln
        last = n
    return b"".join(out)


def device_output(argv, patterns, context, fold, word, line, invert):
    """--device-output --lines: grep -n's stdout from the output library, one device-to-host copy of the finished text."""
    import torch
    rest = [a for a in argv if a not in ("--device-output", "-i", "--ignore-case", "-w", "--word-regexp", "-x", "--line-regexp", "-v", "--invert-match")]
    args, flags = [a for a in rest if not a.startswith("--")], {a for a in rest if a.startswith("--")}
    one_pass = "--one-pass" in flags
    if flags - {"--one-pass"} != {"--lines"} or len(args) != (1 if patterns else 2) or (one_pass and not patterns):
        raise SystemExit("./grep_hip.py --device-output --lines [-i] [-w | -x] [-v] [-A NUM] [-B NUM] [-C NUM] [--one-pass] "
                         "(<needle> | (-e <pattern>)... [-f <patterns file>]) <file>: --device-output writes the text that --lines "
                         "prints, and --one-pass compiles several patterns")
    needles = patterns or [args[0].encode()]
    if word and line:
        raise SystemExit("./grep_hip.py: -w and -x exclude each other (a call keeps whole words or whole lines)")
    if (word or line) and not all(needles):
        raise SystemExit("./grep_hip.py: -w / -x with the empty needle is out of scope (it has no neighbour bytes to test)")
    if len(needles) > ss.ANYOF_MAX_NEEDLES:
        raise SystemExit("./grep_hip.py: %d patterns; a call takes %d (-e / -f)" % (len(needles), ss.ANYOF_MAX_NEEDLES))
    data = open(args[-1], "rb").read()
    hay = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if data else torch.empty(0, dtype=torch.uint8, device="cuda")
    before, after = min(context.get("before", 0), 2 ** 64 - 1), min(context.get("after", 0), 2 ** 64 - 1)
    with ss.output_build():
        if one_pass:
            out = ss.NeedleSet(needles, ignore_case=fold).grep(hay, before, after, line_numbers=True, whole_word=word, whole_line=line, invert=invert)
        elif patterns:
            searchers = [ss.DynamicHipSearcher.new_nocase(p) if fold else ss.DynamicHipSearcher.new(p) for p in needles]
            out = ss.grep_anyof(searchers, hay, before, after, line_numbers=True, ignore_case=fold, whole_word=word, whole_line=line, invert=invert)
        else:
            searcher = ss.DynamicHipSearcher.new_nocase(needles[0]) if fold else ss.DynamicHipSearcher.new(needles[0])
            out = searcher.grep(hay, before, after, line_numbers=True, ignore_case=fold, whole_word=word, whole_line=line, invert=invert)
    sys.stdout.buffer.write(out.cpu().numpy().tobytes())


def leftmost_forms(argv, patterns, context, replace_map, fold, word, line, invert):
    """-o (--count | --offsets) [-i] [-w] (-e NEEDLE ... | -f FILE) FILE: the leftmost-longest, non-overlapping occurrences of a SET of
    needles - byte for byte what LC_ALL=C grep -o -b -F prints for those patterns - and --replace-map MAPFILE [-i] [-w] FILE: the file
    with each of them replaced by its needle's own text, one `needle<TAB>text` pair per line of MAPFILE (ss_find_all_leftmost_set_device
    and ss_replace_set_device of libsliceslice_hip_leftmost.so: the selection and the substitution are made on the device)."""
    what = "--replace-map" if "--replace-map" in argv else "-o"
    usage = ("./grep_hip.py -o (--count | --offsets) [-i] [-w] (-e <needle>)... [-f <needles file>] <file>\n"
             "./grep_hip.py --replace-map <map file> [-i] [-w] <file>")
    refused = [("-x", line), ("-v", invert), (context.get("flag"), bool(context))] + \
              [(f, f in argv) for f in ("--count-lines", "--lines", "--frequencies", "--one-pass", "--device-output", "--replace")] + \
              [(f, f in argv and what == "--replace-map") for f in ("--count", "--offsets", "-o", "--only-matching")] + \
              [("-e / -f", bool(patterns) and what == "--replace-map")]
    for flag, given in refused:
        if given:
            raise SystemExit("./grep_hip.py: %s does not go with %s: the leftmost-longest, non-overlapping selection is about the "
                             "occurrences of a set of needles (-i and -w combine with it)" % (flag, what))
    rest = [a for a in argv if a not in ("-o", "--only-matching", "--replace-map", "-i", "--ignore-case", "-w", "--word-regexp")]
    args, flags = [a for a in rest if not a.startswith("--")], {a for a in rest if a.startswith("--")}
    if len(args) != 1 or (what == "--replace-map" and (replace_map is None or flags)) or (what == "-o" and flags not in ({"--count"}, {"--offsets"})):
        raise SystemExit(usage)
    texts = None
    if what == "--replace-map":
        pairs = [l.split(b"\t", 1) for l in open(replace_map, "rb").read().split(b"\n") if l]
        if not pairs or any(len(p) != 2 for p in pairs):
            raise SystemExit("./grep_hip.py: every line of the map file holds a needle, one TAB and its text")
        patterns, texts = [p[0] for p in pairs], [p[1] for p in pairs]
    if not all(patterns):
        raise SystemExit("./grep_hip.py: the empty needle is out of scope for a set (its occurrences belong to no scan)")
    if len(patterns) > ss.ANYOF_MAX_NEEDLES:
        raise SystemExit("./grep_hip.py: %d needles; a set takes %d" % (len(patterns), ss.ANYOF_MAX_NEEDLES))
    with ss.leftmost_build():
        needles = ss.NeedleSet(patterns, ignore_case=fold)
    import torch
    data = open(args[0], "rb").read()
    hay = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if data else torch.empty(0, dtype=torch.uint8, device="cuda")
    if texts is not None:
        sys.stdout.buffer.write(needles.replace(hay, texts, whole_word=word).cpu().numpy().tobytes())
    elif "--count" in flags:
        print(needles.count_leftmost(hay, whole_word=word))
    else:
        offsets, which = needles.find_all_leftmost(hay, whole_word=word)
        sys.stdout.buffer.write(b"".join(b"%d:%s\n" % (o, data[o:o + len(patterns[k])]) for o, k in zip(offsets.cpu().tolist(), which.cpu().tolist())))


def hex_forms(argv, hex_pattern, patterns, context, replacement, replace_map):
    """--hex PATTERN (--count | --offsets | --count-lines | --lines) [--device-output] FILE: the masked-pattern calls."""
    import torch
    usage = "./grep_hip.py --hex '<pattern>' (--count | --offsets | --count-lines | --lines) [--device-output] <file>"
    args, flags = [a for a in argv if not a.startswith("-")], [a for a in argv if a.startswith("-")]
    device = "--device-output" in flags
    modes = [f for f in flags if f != "--device-output"]
    if hex_pattern is None or len(args) != 1 or len(modes) != 1 or modes[0] not in ("--count", "--offsets", "--count-lines", "--lines") or \
            patterns or context or replacement is not None or replace_map is not None or (device and modes[0] != "--lines"):
        raise SystemExit(usage + ": --hex takes one pattern, one of the four modes and no other flag (--device-output with --lines)")
    data = open(args[0], "rb").read()
    hay = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if data else torch.empty(0, dtype=torch.uint8, device="cuda")
    with ss.masked_build():
        try:
            pat = ss.MaskedPattern.from_hex(hex_pattern)
        except ss.SlicesliceError as e:
            raise SystemExit("./grep_hip.py: --hex %r: %s" % (hex_pattern, e))
        print_pattern_mode(pat, modes[0], device, hay, data)


def print_pattern_mode(pat, mode, device, hay, data):
    """What --count / --offsets / --count-lines / --lines print for a MaskedPattern or a ClassPattern (inside its library's block)."""
    if mode == "--count":
        print(pat.count(hay))
    elif mode == "--offsets":
        sys.stdout.buffer.write(b"".join(b"%d\n" % o for o in pat.find_all(hay).cpu().tolist()))
    elif mode == "--count-lines":
        print(pat.count_lines(hay))
    else:
        begin, end, number = pat.find_lines(hay)
        if device:
            sys.stdout.buffer.write(ss.format_lines(hay, begin, end, number, line_numbers=True).cpu().numpy().tobytes())
        else:
            sys.stdout.buffer.write(b"".join(b"%d:%s\n" % (n, data[b:e]) for b, e, n in zip(begin.cpu().tolist(), end.cpu().tolist(), number.cpu().tolist())))


def classes_forms(argv, class_pattern, patterns, context, replacement, replace_map):
    """--classes PATTERN [-i] (--count | --offsets | --count-lines | --lines) [--device-output] FILE: the byte-class calls."""
    import torch
    usage = "./grep_hip.py --classes '<pattern>' [-i] (--count | --offsets | --count-lines | --lines) [--device-output] <file>"
    args, flags = [a for a in argv if not a.startswith("-")], [a for a in argv if a.startswith("-")]
    device = "--device-output" in flags
    fold = "-i" in flags or "--ignore-case" in flags
    modes = [f for f in flags if f not in ("--device-output", "-i", "--ignore-case")]
    if class_pattern is None or len(args) != 1 or len(modes) != 1 or modes[0] not in ("--count", "--offsets", "--count-lines", "--lines") or \
            patterns or context or replacement is not None or replace_map is not None or (device and modes[0] != "--lines"):
        raise SystemExit(usage + ": --classes takes one pattern, one of the four modes and no other flag but -i (--device-output with --lines)")
    with ss.classes_build():
        try:
            sets = ss.parse_classes(class_pattern, fold)            # (host only: a refused pattern never touches the device)
        except (ss.SlicesliceError, UnicodeEncodeError) as e:
            raise SystemExit("./grep_hip.py: --classes %r: %s" % (class_pattern, e))
        data = open(args[0], "rb").read()
        hay = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if data else torch.empty(0, dtype=torch.uint8, device="cuda")
        try:
            pat = ss.ClassPattern.from_sets(sets)
        except ss.SlicesliceError as e:
            raise SystemExit("./grep_hip.py: --classes %r: %s" % (class_pattern, e))
        print_pattern_mode(pat, modes[0], device, hay, data)


def runs_replace_form(argv, run_pattern, patterns, context, replacement, replace_map):
    """--runs PATTERN [-i] --replace TEXT [--per-line] FILE: the substituted file on stdout (ss.RunPattern.replace)."""
    import torch
    usage = "./grep_hip.py --runs '<pattern>' [-i] --replace <text> [--per-line] <file>"
    args, flags = [a for a in argv if not a.startswith("-")], [a for a in argv if a.startswith("-")]
    fold = "-i" in flags or "--ignore-case" in flags
    listing = [f for f in flags if f in ("--count", "--offsets", "-o", "--count-lines", "--lines")]
    if listing:
        raise SystemExit(usage + ": --replace writes the substituted file and is not combined with %s" % " ".join(listing))
    other = [f for f in flags if f not in ("-i", "--ignore-case", "--replace", "--per-line")]
    if run_pattern is None or replacement is None or len(args) != 1 or other or patterns or context or replace_map is not None:
        raise SystemExit(usage + ": --runs with --replace takes one pattern, one text, one file and no other flag but -i and --per-line")
    with ss.rewrite_build():
        try:
            words, lo, hi = ss.parse_runs(run_pattern, fold)        # (host only: a refused pattern never touches the device)
            text = replacement.encode("latin-1")
        except (ss.SlicesliceError, UnicodeEncodeError) as e:
            raise SystemExit("./grep_hip.py: --runs %r: %s" % (run_pattern, e))
        data = open(args[0], "rb").read()
        hay = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if data else torch.empty(0, dtype=torch.uint8, device="cuda")
        try:
            out = ss.RunPattern.from_set(words, lo, hi).replace(hay, text, b"\n" if "--per-line" in flags else None)
        except ss.SlicesliceError as e:
            raise SystemExit("./grep_hip.py: --runs %r --replace: %s" % (run_pattern, e))
        sys.stdout.buffer.write(out.cpu().numpy().tobytes())


def runs_forms(argv, run_pattern, patterns, context, replacement, replace_map):
    """--runs PATTERN [-i] (--count | --offsets | -o | --count-lines | --lines) [--device-output] FILE: the run calls."""
    import torch
    if replacement is not None or "--replace" in argv or "--per-line" in argv:
        return runs_replace_form(argv, run_pattern, patterns, context, replacement, replace_map)
    usage = "./grep_hip.py --runs '<pattern>' [-i] (--count | --offsets | -o | --count-lines | --lines) [--device-output] <file>"
    args, flags = [a for a in argv if not a.startswith("-")], [a for a in argv if a.startswith("-")]
    device = "--device-output" in flags
    fold = "-i" in flags or "--ignore-case" in flags
    modes = [f for f in flags if f not in ("--device-output", "-i", "--ignore-case")]
    if run_pattern is None or len(args) != 1 or len(modes) != 1 or modes[0] not in ("--count", "--offsets", "-o", "--count-lines", "--lines") or \
            patterns or context or replacement is not None or replace_map is not None or (device and modes[0] != "--lines"):
        raise SystemExit(usage + ": --runs takes one pattern, one of the five modes and no other flag but -i (--device-output with --lines)")
    with ss.runs_build():
        try:
            words, lo, hi = ss.parse_runs(run_pattern, fold)        # (host only: a refused pattern never touches the device)
        except (ss.SlicesliceError, UnicodeEncodeError) as e:
            raise SystemExit("./grep_hip.py: --runs %r: %s" % (run_pattern, e))
        data = open(args[0], "rb").read()
        hay = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if data else torch.empty(0, dtype=torch.uint8, device="cuda")
        pat = ss.RunPattern.from_set(words, lo, hi)
        if modes[0] == "--offsets":
            begin, end = pat.find_all(hay)
            sys.stdout.buffer.write(b"".join(b"%d:%d\n" % (b, e) for b, e in zip(begin.cpu().tolist(), end.cpu().tolist())))
        elif modes[0] == "-o":
            begin, end = pat.find_all(hay)
            if begin.numel():
                sys.stdout.buffer.write(ss.gather_ranges(hay, begin, end, b"\n").cpu().numpy().tobytes())
        else:
            print_pattern_mode(pat, modes[0], device, hay, data)


def fields_form(argv, field_list, separator):
    """--fields LIST -d SEP [--merge] [-s] [--device-output] FILE: the selected fields, one line per record (ss.FieldSelector)."""
    import torch
    usage = "./grep_hip.py --fields <list> -d <sep> [--merge] [-s] [--device-output] <file>"
    args, flags = [a for a in argv if not a.startswith("-")], [a for a in argv if a.startswith("-")]
    other = [f for f in flags if f not in ("--merge", "-s", "--device-output")]
    if field_list is None or not separator or len(args) != 1 or other:
        raise SystemExit(usage + ": --fields takes one range, one separator, one file and no other flag but --merge, -s and --device-output")
    with ss.fields_build():
        try:
            first, last = ss.parse_fields(field_list)               # (host only: a refused list never touches the device)
            sep = separator.encode("latin-1") if len(separator) == 1 else separator
            sel = ss.FieldSelector(sep, first, last, merge="--merge" in flags, keep_short="-s" not in flags)
        except (ss.SlicesliceError, UnicodeEncodeError, ValueError) as e:
            raise SystemExit("./grep_hip.py: --fields %r -d %r: %s" % (field_list, separator, e))
        data = open(args[0], "rb").read()
        hay = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if data else torch.empty(0, dtype=torch.uint8, device="cuda")
        if "--device-output" in flags:
            sys.stdout.buffer.write(sel.cut(hay).cpu().numpy().tobytes())
        else:
            begin, end, _ = sel.find(hay)
            sys.stdout.buffer.write(b"".join(data[b:e] + b"\n" for b, e in zip(begin.cpu().tolist(), end.cpu().tolist())))


def print_groups(hay, data, begin, end, count, device, counted=True):
    """`count<TAB>key` per row (counted=False: the key alone).  device: the keys are gathered on the device (ss.gather_ranges) and come
    to the host in one copy with their starts; otherwise the rows come and the host slices the file."""
    if begin.numel() == 0:
        return
    counts = count.cpu().tolist()
    if device:
        text, starts = ss.gather_ranges(hay, begin, end, b"\n", return_starts=True)
        if not counted:
            sys.stdout.buffer.write(text.cpu().numpy().tobytes())
            return
        text, starts = text.cpu().numpy().tobytes(), starts.cpu().tolist()
        keys = (text[starts[k]:starts[k + 1]] for k in range(len(counts)))
    else:
        keys = (data[b:e] + b"\n" for b, e in zip(begin.cpu().tolist(), end.cpu().tolist()))
    sys.stdout.buffer.write(b"".join(key if not counted else b"%d\t%s" % (c, key) for c, key in zip(counts, keys)))


def top_amount(text):
    if text is None or not (text.isascii() and text.isdigit()):
        raise SystemExit("./grep_hip.py: --top takes a non-negative integer (a number of rows), got %r" % (text,))
    return int(text)


def groups_forms(argv, run_pattern, top):
    """--runs PATTERN --uniq-count [-i] [--top K] [--device-output] FILE, --lines-uniq-count [-i] [--top K] [--device-output] FILE and
    --uniq [-i] [--device-output] FILE: the grouping calls (ss.RunPattern.groups / most_common, ss.group_lines)."""
    import torch
    usage = ("./grep_hip.py --runs '<pattern>' --uniq-count [-i] [--top <k>] [--device-output] <file>\n"
             "./grep_hip.py (--lines-uniq-count [--top <k>] | --uniq) [-i] [--device-output] <file>")
    args, flags = [a for a in argv if not a.startswith("-")], [a for a in argv if a.startswith("-")]
    device = "--device-output" in flags
    fold = "-i" in flags or "--ignore-case" in flags
    modes = [f for f in flags if f not in ("--device-output", "-i", "--ignore-case")]
    if len(args) != 1 or len(modes) != 1 or (modes[0] == "--uniq-count") != (run_pattern is not None) or (modes[0] == "--uniq" and top is not None):
        raise SystemExit(usage + ": one mode, one file; --uniq-count goes with --runs, the two line modes without; --top not with --uniq")
    with ss.groups_build():
        data = open(args[0], "rb").read()
        hay = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if data else torch.empty(0, dtype=torch.uint8, device="cuda")
        if run_pattern is not None:
            try:
                words, lo, hi = ss.parse_runs(run_pattern, fold)    # (host only: a refused pattern never touches the device)
            except (ss.SlicesliceError, UnicodeEncodeError) as e:
                raise SystemExit("./grep_hip.py: --runs %r: %s" % (run_pattern, e))
            pat = ss.RunPattern.from_set(words, lo, hi)
            begin, end, count = pat.groups(hay, ignore_case=fold) if top is None else pat.most_common(hay, top, ignore_case=fold)
        else:
            begin, end, _, count = ss.group_lines(hay, ignore_case=fold)
            if top is not None:
                order = torch.sort(count, descending=True, stable=True).indices[:top]
                begin, end, count = begin[order], end[order], count[order]
        print_groups(hay, data, begin, end, count, device, counted=modes[0] != "--uniq")


def main():
    if "--help" in sys.argv[1:]:
        print(__doc__)
        return None
    argv, patterns, context, replacement, replace_map = [], [], {}, None, None
    top = None
    run_pattern, runs_given = None, False
    field_list, fields_given, separator = None, False, None
    hex_pattern, hex_given = None, False
    class_pattern, classes_given = None, False
    it = iter(sys.argv[1:])
    for a in it:
        if a == "--replace":
            argv.append(a)
            replacement = next(it, None)
        elif a == "--replace-map":
            argv.append(a)
            replace_map = next(it, None)
        elif a == "--hex":
            hex_given, hex_pattern = True, next(it, None)
        elif a == "--classes":
            classes_given, class_pattern = True, next(it, None)
        elif a == "--runs":
            runs_given, run_pattern = True, next(it, None)
        elif a == "--top":
            top = top_amount(next(it, None))
        elif a == "--fields":
            fields_given, field_list = True, next(it, None)
        elif a == "-d" and "--fields" in sys.argv:
            separator = next(it, None)
        elif a == "-e":
            patterns.append(next(it).encode())
        elif a == "-f":
            patterns += [l for l in open(next(it), "rb").read().split(b"\n") if l]
        elif a in _CONTEXT_FLAGS or a[:2] in ("-A", "-B", "-C") or a.split("=", 1)[0] in _CONTEXT_FLAGS:
            if a in _CONTEXT_FLAGS:
                flag, text = a, next(it, "")
            elif a.startswith("--"):
                flag, text = a.split("=", 1)
            else:
                flag, text = a[:2], a[2:]
            amount = context_amount(flag, text)
            for side in ("before", "after"):
                if _CONTEXT_FLAGS[flag] in (side, "both"):
                    context[side] = amount
            context["flag"] = flag
        else:
            argv.append(a)
    if hex_given + classes_given + runs_given > 1:
        raise SystemExit("./grep_hip.py: --hex, --classes and --runs are three pattern languages: give one")
    if "--uniq-count" in argv or "--lines-uniq-count" in argv or "--uniq" in argv:
        if hex_given or classes_given or fields_given or patterns or context or replacement is not None or replace_map is not None:
            raise SystemExit("./grep_hip.py: --uniq-count, --lines-uniq-count and --uniq group tokens or lines and are not combined with "
                             "--hex, --classes, --fields, context, -e / -f or --replace")
        if runs_given and run_pattern is None:
            raise SystemExit("./grep_hip.py: --runs takes a pattern")
        return groups_forms(argv, run_pattern if runs_given else None, top)
    if top is not None:
        raise SystemExit("./grep_hip.py: --top goes with --uniq-count or --lines-uniq-count")
    if fields_given:
        if hex_given or classes_given or runs_given or patterns or context or replacement is not None or replace_map is not None:
            raise SystemExit("./grep_hip.py: --fields selects columns and is not combined with a pattern, context, -e / -f or --replace")
        return fields_form(argv, field_list, separator)
    if runs_given:
        return runs_forms(argv, run_pattern, patterns, context, replacement, replace_map)
    if hex_given:
        return hex_forms(argv, hex_pattern, patterns, context, replacement, replace_map)
    if classes_given:
        return classes_forms(argv, class_pattern, patterns, context, replacement, replace_map)
    fold = "-i" in argv or "--ignore-case" in argv
    word = "-w" in argv or "--word-regexp" in argv
    line = "-x" in argv or "--line-regexp" in argv
    invert = "-v" in argv or "--invert-match" in argv
    only = "-o" in argv or "--only-matching" in argv
    if "--device-output" in argv and not (only or "--replace" in argv or "--frequencies" in argv):
        return device_output(argv, patterns, context, fold, word, line, invert)
    if "--replace-map" in argv or (only and patterns and "--replace" not in argv and "--frequencies" not in argv):
        return leftmost_forms(argv, patterns, context, replace_map, fold, word, line, invert)
    if only or "--replace" in argv:
        what = "--replace" if "--replace" in argv else "-o"
        usage = ("./grep_hip.py -o (--count | --offsets) [-i] [-w] <needle> <file>\n"
                 "./grep_hip.py --replace <text> [-i] [-w] <needle> <file>")
        refused = [("-x", line), ("-v", invert), (context.get("flag"), bool(context))] + \
                  [(f, f in argv) for f in ("--count-lines", "--lines", "--frequencies", "--one-pass")] + [("-e / -f", bool(patterns))] + \
                  [(f, f in argv and what == "--replace") for f in ("--count", "--offsets", "-o", "--only-matching")]
        for flag, given in refused:
            if given:
                raise SystemExit("./grep_hip.py: %s does not go with %s: the non-overlapping selection is about the occurrences of one "
                                 "needle (-i and -w combine with it)" % (flag, what))
        rest = [a for a in argv if a not in ("-o", "--only-matching", "--replace", "-i", "--ignore-case", "-w", "--word-regexp")]
        args, flags = [a for a in rest if not a.startswith("--")], {a for a in rest if a.startswith("--")}
        if len(args) != 2 or (what == "--replace" and (replacement is None or flags)) or (what == "-o" and flags not in ({"--count"}, {"--offsets"})):
            raise SystemExit(usage)
        needle = args[0].encode()
        if not needle and (what == "--replace" or fold or word):
            raise SystemExit("./grep_hip.py: the empty needle cannot be replaced, folded or stand as a word (non-overlapping forms)")
        with ss.disjoint_build():
            searcher = ss.DynamicHipSearcher.new_nocase(needle) if fold else ss.DynamicHipSearcher.new(needle)
        import torch
        data = open(args[1], "rb").read()
        hay = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda() if data else torch.empty(0, dtype=torch.uint8, device="cuda")
        if what == "--replace":
            sys.stdout.buffer.write(searcher.replace(hay, replacement.encode(), ignore_case=fold, whole_word=word).cpu().numpy().tobytes())
        elif "--count" in flags:
            print(searcher.count_disjoint(hay, ignore_case=fold, whole_word=word))
        else:
            n = len(needle)
            sys.stdout.buffer.write(b"".join(b"%d:%s\n" % (o, data[o:o + n])
                                             for o in searcher.find_all_disjoint(hay, ignore_case=fold, whole_word=word).cpu().tolist()))
        return
    if "--frequencies" in argv:
        rest = [a for a in argv if a not in ("--frequencies", "-i", "--ignore-case", "-w", "--word-regexp")]
        if line:
            raise SystemExit("./grep_hip.py: -x is about lines, and --frequencies counts occurrences, which know no line")
        if invert:
            raise SystemExit("./grep_hip.py: -v is about lines: --frequencies counts occurrences, which have no complement")
        if context:
            raise SystemExit("./grep_hip.py: %s adds context LINES: --frequencies counts occurrences and prints numbers" % context["flag"])
        if not patterns or len(rest) != 1 or rest[0].startswith("--"):
            raise SystemExit("./grep_hip.py --frequencies [-i] [-w] (-e <pattern>)... [-f <patterns file>] <file>")
        if not all(patterns):
            raise SystemExit("./grep_hip.py: --frequencies with the empty pattern is out of scope (its occurrences belong to no scan)")
        if len(patterns) > ss.ANYOF_MAX_NEEDLES:
            raise SystemExit("./grep_hip.py: %d patterns; a set takes %d (-e / -f)" % (len(patterns), ss.ANYOF_MAX_NEEDLES))
        with ss.setmatches_build():
            needles = ss.NeedleSet(patterns, ignore_case=fold)
        data = open(rest[0], "rb").read()
        sys.stdout.write("".join("%d\n" % c for c in needles.count(data, whole_word=word).cpu().tolist()))
        return
    one_pass = "--one-pass" in argv
    argv = [a for a in argv if a != "--one-pass"]
    if one_pass and not (patterns and {"--count-lines", "--lines"} & set(argv) and not {"--count", "--offsets"} & set(argv)):
        raise SystemExit("./grep_hip.py: --one-pass compiles several patterns into one set: it goes with -e / -f and --count-lines or "
                         "--lines only")
    argv = [a for a in argv if a not in ("-i", "--ignore-case", "-w", "--word-regexp", "-x", "--line-regexp", "-v", "--invert-match")]
    args = [a for a in argv if not a.startswith("--")]
    flags = {a for a in argv if a.startswith("--")}
    if patterns and flags & {"--count-lines", "--lines"} and not flags & {"--count", "--offsets"}:
        if len(args) != 1 or len(flags) != 1:
            raise SystemExit("./grep_hip.py (--count-lines | --lines) [-i] [-w | -x] [-v] [-A NUM] [-B NUM] [-C NUM] (-e <pattern>)... "
                             "[-f <patterns file>] <file>")
        if context and "--lines" not in flags:
            raise SystemExit("./grep_hip.py: %s adds context LINES to the lines that --lines prints: it goes with --lines only; "
                             "--count-lines prints a number" % context["flag"])
        if word and line:
            raise SystemExit("./grep_hip.py: -w and -x exclude each other (a call keeps whole words or whole lines)")
        if (word or line) and not all(patterns):
            raise SystemExit("./grep_hip.py: -w / -x with the empty needle is out of scope (it has no neighbour bytes to test)")
        if len(patterns) > ss.ANYOF_MAX_NEEDLES:
            raise SystemExit("./grep_hip.py: %d patterns; a call takes %d (-e / -f)" % (len(patterns), ss.ANYOF_MAX_NEEDLES))
        if one_pass:
            with ss.needleset_build():
                needles = ss.NeedleSet(patterns, ignore_case=fold)
            data = open(args[0], "rb").read()
            if "--lines" in flags:
                sys.stdout.buffer.write(context_lines(needles, data, context.get("before", 0), context.get("after", 0), invert=invert,
                                                      whole_word=word, whole_line=line))
            else:
                print(needles.count_lines(data, invert=invert, whole_word=word, whole_line=line))
            return
        with ss.anyof_build():
            searchers = [ss.DynamicHipSearcher.new_nocase(p) if fold else ss.DynamicHipSearcher.new(p) for p in patterns]
        data = open(args[0], "rb").read()
        if "--lines" in flags:
            sys.stdout.buffer.write(context_lines(searchers, data, context.get("before", 0), context.get("after", 0), ignore_case=fold,
                                                  invert=invert, whole_word=word, whole_line=line))
        else:
            print(ss.count_lines_anyof(searchers, data, ignore_case=fold, invert=invert, whole_word=word, whole_line=line))
        return
    if patterns:
        if invert:
            raise SystemExit("./grep_hip.py: -v is not available with -e / -f: several patterns go through the batched library, which "
                             "counts occurrences, and occurrences have no complement - run one pattern per call with --count-lines, or give --count-lines / --lines "
                             "with the patterns (the lines that match none of them)")
        if word or line:
            raise SystemExit("./grep_hip.py: -w / -x are not available with -e / -f: several patterns go through the batched library, "
                             "which has no whole-word form - run one pattern per call")
        if fold:
            raise SystemExit("./grep_hip.py: -i is not available with -e / -f: several patterns go through the batched library, "
                             "which has no case-folding form - run one pattern per call")
        if context:
            raise SystemExit("./grep_hip.py: %s is not available with -e / -f: several patterns go through the batched library, which "
                             "counts occurrences and knows no lines - run one pattern per call with --lines" % context["flag"])
        if len(args) != 1 or flags != {"--count"}:
            raise SystemExit("./grep_hip.py --count (-e <pattern>)... [-f <patterns file>] <file>")
        sys.stdout.write("".join("%d\n" % c for c in count_patterns(patterns, args[0])))
        return
    if len(args) < 2 or flags - {"--count", "--offsets", "--count-lines", "--lines", "--rare-position"}:
        raise SystemExit("./grep_hip.py [-i | --ignore-case] [-w | --word-regexp | -x | --line-regexp] [-v | --invert-match] "
                         "[-A NUM | --after-context=NUM] [-B NUM | --before-context=NUM] [-C NUM | --context=NUM] <needle> "
                         "<file> [--count | --offsets | --count-lines | --lines]")
    needle, filename = args[0].encode(), args[1]
    if context:
        if flags & {"--count", "--offsets", "--count-lines"} or "--lines" not in flags:
            raise SystemExit("./grep_hip.py: %s adds context LINES to the lines that --lines prints: it goes with --lines only; --count, "
                             "--offsets and --count-lines print numbers, and the plain search prints one word" % context["flag"])
        if word and line:
            raise SystemExit("./grep_hip.py: -w and -x exclude each other (a call keeps whole words or whole lines)")
        if (word or line) and not needle:
            raise SystemExit("./grep_hip.py: -w / -x with the empty needle is out of scope (it has no neighbour bytes to test)")
        with ss.context_build():
            searcher = ss.DynamicHipSearcher.new_nocase(needle) if fold else ss.DynamicHipSearcher.new(needle)
        data = open(filename, "rb").read()
        sys.stdout.buffer.write(context_lines(searcher, data, context.get("before", 0), context.get("after", 0), ignore_case=fold,
                                              invert=invert, whole_word=word, whole_line=line))
        return
    if invert:
        if flags & {"--count", "--offsets"} or not flags & {"--count-lines", "--lines"}:
            raise SystemExit("./grep_hip.py: -v is about lines: it goes with --count-lines or --lines; --count and --offsets are about "
                             "occurrences, which have no complement")
        if word and line:
            raise SystemExit("./grep_hip.py: -w and -x exclude each other (a call keeps whole words or whole lines)")
        if (word or line) and not needle:
            raise SystemExit("./grep_hip.py: -w / -x with the empty needle is out of scope (it has no neighbour bytes to test)")
        with ss.inverted_build():
            searcher = ss.DynamicHipSearcher.new_nocase(needle) if fold else ss.DynamicHipSearcher.new(needle)
        data = open(filename, "rb").read()
        if "--lines" in flags:
            for n, text in matching_lines(searcher, data, ignore_case=fold, invert=True, whole_word=word, whole_line=line):
                sys.stdout.buffer.write(b"%d:%s\n" % (n, text))
        else:
            print(searcher.count_lines_inverted(data, ignore_case=fold, whole_word=word, whole_line=line))
        return
    if word or line:
        if word and line:
            raise SystemExit("./grep_hip.py: -w and -x exclude each other (a call keeps whole words or whole lines)")
        if not flags & {"--count", "--offsets", "--count-lines", "--lines"}:
            raise SystemExit("./grep_hip.py: -w / -x need one of --count, --offsets, --count-lines, --lines (the early-exit search has "
                             "no whole-word form)")
        if line and not flags & {"--count-lines", "--lines"}:
            raise SystemExit("./grep_hip.py: -x is about lines: it goes with --count-lines or --lines, not with the occurrence outputs")
        if not needle:
            raise SystemExit("./grep_hip.py: -w / -x with the empty needle is out of scope (it has no neighbour bytes to test)")
        bound = dict(whole_word=word, whole_line=line) if flags & {"--count-lines", "--lines"} else dict(whole_word=word)
        with ss.bounded_build():
            searcher = ss.DynamicHipSearcher.new_nocase(needle) if fold else ss.DynamicHipSearcher.new(needle)
        data = open(filename, "rb").read()
        if "--lines" in flags:
            for n, text in matching_lines(searcher, data, ignore_case=fold, **bound):
                sys.stdout.buffer.write(b"%d:%s\n" % (n, text))
        elif "--count-lines" in flags:
            print(searcher.count_lines(data, ignore_case=fold, **bound))
        elif "--offsets" in flags:
            sys.stdout.write("".join("%d\n" % o for o in searcher.find_all(data, ignore_case=fold, **bound).cpu().tolist()))
        else:
            print(searcher.count(data, ignore_case=fold, **bound))
        return
    if fold:
        if not flags & {"--count", "--offsets", "--count-lines", "--lines"}:
            raise SystemExit("./grep_hip.py: -i needs one of --count, --offsets, --count-lines, --lines (the early-exit search has no "
                             "case-folding form)")
        with ss.nocase_build():
            searcher = ss.DynamicHipSearcher.new_nocase(needle)
        data = open(filename, "rb").read()
        if "--lines" in flags:
            for n, line in matching_lines(searcher, data, ignore_case=True):
                sys.stdout.buffer.write(b"%d:%s\n" % (n, line))
        elif "--count-lines" in flags:
            print(searcher.count_lines(data, ignore_case=True))
        elif "--offsets" in flags:
            sys.stdout.write("".join("%d\n" % o for o in searcher.find_all(data, ignore_case=True).cpu().tolist()))
        else:
            print(searcher.count(data, ignore_case=True))
        return
    if "--count-lines" in flags or "--lines" in flags:
        with ss.lines_build():
            searcher = ss.DynamicHipSearcher.new(needle)
        data = open(filename, "rb").read()
        if "--lines" in flags:
            for n, line in matching_lines(searcher, data):
                sys.stdout.buffer.write(b"%d:%s\n" % (n, line))
        else:
            print(searcher.count_lines(data))
        return
    if "--count" in flags or "--offsets" in flags:
        with ss.matches_build():
            searcher = ss.DynamicHipSearcher.new(needle)
        data = open(filename, "rb").read()
        if "--offsets" in flags:
            sys.stdout.write("".join("%d\n" % o for o in searcher.find_all(data).cpu().tolist()))
        else:
            print(searcher.count(data))
        return
    searcher = ss.DynamicHipSearcher.new(needle)
    print("Searching for %s in %r: %s" % (args[0], filename, str(ss.search_file(searcher, filename)).lower()))


if __name__ == "__main__":
    main()

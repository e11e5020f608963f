#!/usr/bin/env python3
"""./grep_hip.py <needle> <file> [--count | --offsets] - the reference's examples/grep.rs:42-56 with the "hip"
backend: map the file, build one searcher, one search_in, print the boolean.
  --count    grep -c style: the number of (overlapping) occurrences (libsliceslice_hip_matches.so, ss_count_device)
  --offsets  grep -b -o style: one byte offset per line, ascending (ss_find_all_device)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sliceslice_rs_amd as ss  # noqa: E402


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    flags = {a for a in sys.argv[1:] if a.startswith("--")}
    if len(args) < 2 or flags - {"--count", "--offsets", "--rare-position"}:
        raise SystemExit("./grep_hip.py <needle> <file> [--count | --offsets]")
    needle, filename = args[0].encode(), args[1]
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

"""Regenerates tests/golden/regex_compiled.json: the compiled form (or the refusal) of every pattern of tests/test_regex_compiled.py::cases(),
as hmse_amd/regex.py compiles it NOW.  The fixture pins the compiler across refactors, so record it before the compiler is touched and
read a diff of it as a change of the compiled form.  Run from the repo root:  python tests/golden/make_regex_compiled.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_regex_compiled as T  # noqa: E402


def main():
    entries = [T.compiled(p, fl) for p, fl in T.cases()]
    with open(os.path.join(HERE, "regex_compiled.json"), "w") as f:
        f.write('{"fields": %s,\n "entries": [\n' % json.dumps(T.FIELDS))
        f.write(",\n".join(json.dumps(e, separators=(",", ":")) for e in entries))
        f.write("\n]}\n")
    print(f"{len(entries)} entries, {sum(1 for e in entries if len(e) == 3)} of them refusals")


if __name__ == "__main__":
    main()

"""CPU: the compiled form of hmse_amd.regex.Regex is pinned.  tests/golden/regex_compiled.json (written by tests/golden/make_regex_compiled.py)
holds, for every pattern of cases(), its sizes, its start states and a hash of its class map and table — or the text of its refusal — and
every one must compile to exactly that: a change to the compiler that renumbers a state, merges a class differently or words a refusal
differently shows here, whichever form (plain or asserting) it touches."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "regex_compiled.json")
IC, DOTALL, ASSERTIONS = 1, 2, 4                                   # the flag bits of an entry
FIELDS = ["pattern (hex)", "flags: 1 ignore_case | 2 dotall | 4 assertions",
          "[n_states, n_classes, reach, min_len], or the RegexError's text", "start", "sha256(classmap bytes + table bytes)[:16]"]


def cases():
    """[(pattern, flags)], without duplicates: the hand-picked sizes, both emulators' automata, every refusal of the two host test files
    that is a bytes pattern (a str or an int has no hex form), the first 60 generated patterns under the four flag pairs, and what
    tests/test_regexa_host.py compiles with assertions."""
    import test_regex_host as H
    import test_regexa_host as A
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import regex_emu
    import regexa_emu
    out = [(s[0], 0) for s in H.SIZES]
    out += [(p, fl) for p, fl in regex_emu.PATTERNS] + [(p, fl | ASSERTIONS) for p, fl in regexa_emu.PATTERNS]
    # refusals, plain: the syntax, the caps, the empty languages, and what only assertions=True takes
    out += [(p, 0) for p, _ in H.REFUSED]
    out += [(p, 0) for p in (b"(a|b)*a(a|b){13}", b"(a|b)*a(a|b){11}", b"a{200}b{57}", b"a{200}b{56}", b"", b"()", b"(|)", b"a{0}", b"(a{0,0})*")]
    out += [(p, 0) for p in (b"^a", b"a$", b"a|^b", rb"\ba", rb"a\Z")]
    # refusals, asserting
    out += [(p, ASSERTIONS) for p in (rb"^*a", rb"a\b+", rb"a$?", rb"\B{2}a", rb"a[\b]", rb"a\z", rb"\Ga", rb"a(?=b)", rb"(?<!a)b", rb"(?m)^a", rb"^a(", rb"a\Z*")]
    out += [(p, ASSERTIONS) for p in (rb"a^b", rb"^$", rb"\b\B.", rb"a\Ab", rb"\Z.", rb"(^|$)", rb"\w\b\w")]
    out += [(p, ASSERTIONS) for p in (rb"\b[a-z]{200,256}\b", rb"^[ab]*a[ab]{11}$", rb"^(abcdefghijklmnopq){256}$", rb"^a{256}b")]
    rng = np.random.default_rng(7)
    for _ in range(60):
        p, _ = H.gen(rng, 3, H.BUDGET)
        out += [(p, fl) for fl in (0, IC, DOTALL, IC | DOTALL)]
    built = [q for x in A.ASSERTIONS for q in A._built(x)]
    out += [(p, fl | ASSERTIONS) for p in built for fl in (0, IC)]
    out += [(p, fl | ASSERTIONS) for p in A.GROUPS for fl in (0, IC, DOTALL, IC | DOTALL)]
    out += [(p, ASSERTIONS) for p in (rb"\bcat\b", rb"^ERROR", rb";$", rb"\A\w+|\w+\Z", rb"\Aab", rb"(^|b)a\b", rb"a{256}$", rb"a{256}\b", rb"a{255}\B", rb"q+\b",
                                      rb"(^|,)*a", rb"(\b)+a", rb"\^a\$")]
    out.append((rb"\Aa|^b|\Bc|\b-", ASSERTIONS))                   # (none of the above has four distinct start states)
    for p, ic, dotall in ((b"ab", 0, 0), (b"a+b*", IC, 0), (rb"[ab]{2,5}", 0, 0), (rb"a.{0,7}b", 0, DOTALL), (rb"\w+\s", 0, 0), (rb"(ab|b)c?", IC, 0),
                          (rb"[^\n]*c", 0, 0), (rb"b{255}a", 0, 0), (rb".", 0, 0)):
        out += [(p, ic | dotall), (p, ic | dotall | ASSERTIONS)]
    return list(dict.fromkeys(out))


def compiled(pattern, flags):
    """one entry of the fixture"""
    from hmse_amd.regex import Regex, RegexError
    head = [pattern.hex(), flags]
    try:
        r = Regex(pattern, bool(flags & IC), bool(flags & DOTALL), assertions=bool(flags & ASSERTIONS))
    except RegexError as e:
        return head + [str(e)]
    digest = hashlib.sha256(r.classmap.tobytes() + r.table.tobytes()).hexdigest()[:16]
    return head + [[int(r.n_states), int(r.n_classes), int(r.reach), int(r.min_len)], [int(s) for s in r.start], digest]


def test_every_pattern_compiles_to_its_recorded_form():
    fixture = json.load(open(FIXTURE))
    assert fixture["fields"] == FIELDS
    pinned = {(e[0], e[1]): e for e in fixture["entries"]}
    want = cases()
    assert len(pinned) == len(fixture["entries"]) and sorted(pinned) == sorted((p.hex(), fl) for p, fl in want)      # none missing, none left over
    for p, fl in want:
        assert compiled(p, fl) == pinned[(p.hex(), fl)], (p, fl)
    forms = [e for e in fixture["entries"] if len(e) == 5]
    refused = [e for e in fixture["entries"] if len(e) == 3]
    assert len(forms) > 400 and len(refused) > 80
    asserting = [e for e in forms if e[1] & ASSERTIONS]
    assert any(e[2][2] == 256 for e in asserting) and any(len(set(e[3])) == 4 for e in asserting)     # a cyclic one; four distinct starts
    e = pinned[(rb"\Aab".hex(), ASSERTIONS)]
    assert e[3][0] != e[3][1] == e[3][2] == e[3][3]                                                   # the starts that keep a zero row
    assert all(e[3] == [1, 1, 1, 1] for e in forms if not e[1] & ASSERTIONS)
    assert os.path.getsize(FIXTURE) <= 48 * 1024

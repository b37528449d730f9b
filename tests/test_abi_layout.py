"""Host: the Python mirrors of include/hmse.h agree with the header — the layout of the three structs that cross the boundary
(hmse_cfg, hmse_gl4, hmse_stream) as the C compiler lays them out, and every named word and status bit of the streaming state block."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hmse.h")


def _mirrors():
    from hmse_amd import _lib
    return {"hmse_cfg": _lib.HmseCfg, "hmse_gl4": _lib.HmseGl4, "hmse_stream": _lib.HmseStream}


def _struct_fields(header: str, name: str) -> list:
    """Field names of `typedef struct <name> { ... } <name>;` in declaration order (comments dropped; `a, b` and `T* a; T b;` lines)."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            fields += [d.split()[-1].lstrip("*") for d in decl.split(",")]
    return fields


def test_struct_mirrors_have_the_layout_the_c_compiler_gives_the_header(tmp_path):
    """sizeof and every offsetof of the three structs, printed by a C99 program that includes the header, against ctypes."""
    with open(HEADER) as f:
        header = f.read()
    mirrors = _mirrors()
    fields = {name: _struct_fields(header, name) for name in mirrors}
    for name, m in mirrors.items():
        assert fields[name] == [f[0] for f in m._fields_], name       # same names, same order
    lines = ['#include <stdio.h>', '#include "hmse.h"', 'int main(void) {']
    for name, fs in fields.items():
        lines.append(f'  printf("{name} sizeof %zu\\n", sizeof({name}));')
        lines += [f'  printf("{name} {f} %zu\\n", offsetof({name}, {f}));' for f in fs]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)])
    got = [ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines()]
    assert len(got) == sum(len(fs) + 1 for fs in fields.values())
    for name, what, value in got:
        m = mirrors[name]
        assert int(value) == (C.sizeof(m) if what == "sizeof" else getattr(m, what).offset), (name, what)
    assert C.sizeof(mirrors["hmse_cfg"]) == 64 and C.sizeof(mirrors["hmse_gl4"]) == 136


def _header_constants(prefix: str) -> dict:
    """NAME -> value of every `PREFIX_NAME = <int>` enumerator and `#define PREFIX_NAME <int expression>` of the header."""
    with open(HEADER) as f:
        header = f.read()
    found = re.findall(r"^\s*(?:#define\s+)?%s(\w+)\s*=?\s*(\(?[0-9][0-9ul <]*\)?)\s*,?\s*(?:/\*|$)" % prefix, header, re.M)
    return {name: eval(re.sub(r"[ul]", "", value)) for name, value in found}


def test_state_words_and_status_bits_equal_the_header_s():
    from hmse_amd import stream_common as sc
    words = _header_constants("HMSE_SB_")
    assert set(words) == {"OFF", "N_OLD", "N_NEW", "U_OLD", "U_NEW", "S_OLD", "S_NEW", "STATUS", "G_OLD", "G_NEW", "G_BASE", "WORDS"}
    for name, value in words.items():
        assert getattr(sc, "SB_" + name) == value, name
    bits = _header_constants("HMSE_STREAM_ST_")
    assert bits == {"CHUNK_CAP": 1, "STORED_CAP": 2, "L2": 4, "ROW": 8, "WS_INIT": 16, "STATE": 32, "PUSH_REFUSED": 64, "SIG_ROW": 128,
                    "DEFLATE_SHIFT": 8, "HOST_REFUSED": 1 << 16}
    for name, value in bits.items():
        assert getattr(sc, "ST_" + name) == value, name
    # the text of the status names every bit through one table, which holds no bit the header does not have
    assert {(name, bit) for bit, name, _ in sc.STATUS_BITS} == {(n, v) for n, v in bits.items() if n != "DEFLATE_SHIFT"}
    req = _header_constants("HMSE_GL4_REQ_")
    assert req == {"TOTAL": 0, "STORED": 1, "EXTRA": 2}
    assert (sc.GL4_REQ_TOTAL, sc.GL4_REQ_STORED, sc.GL4_REQ_EXTRA) == (0, 1, 2)


@pytest.mark.parametrize("host_refused", [False, True])
def test_the_status_text_names_every_bit(host_refused):
    from hmse_amd import stream_common as sc
    every = sum(bit for bit, _, _ in sc.STATUS_BITS) | 0x1F << sc.ST_DEFLATE_SHIFT
    status = every if host_refused else every & ~sc.ST_HOST_REFUSED
    msg = str(sc.chain_status_error(status, " on some rank", "the reason", intact=" (tail)"))
    assert msg.startswith(f"streaming chain status {status:#x} on some rank: bit0 chunk capacity, bit1 stored-chunk capacity, bit2 L2 (")
    for bit, _, text in sc.STATUS_BITS:
        assert f"bit{bit.bit_length() - 1} {text}" in msg, bit
    assert "bits 8..12 DEFLATE (0x100 stream capacity, 0x200 workspace), bit16 " in msg
    # the rank's own reason stands behind the bit this rank set: bit 16 if that is up, else bit 6 — once
    assert msg.count("(this rank: the reason)") == 1
    behind = sc.STATUS_BITS[-1][2] if host_refused else "a piece refused by push()"
    assert behind + " (this rank: the reason)" in msg
    assert msg.endswith("; the failing batch and every later one were dropped (tail)")
    assert "this rank" not in str(sc.chain_status_error(status))

"""CPU tests of the saved-model reader (ocffm_model_file_info /
ocffm.model_file_info): files written by hand here, a small text model and its
binary twin built with struct.pack.  No GPU: the reader is host code and
touches no device.  The same files go through a stand-alone driver of the
reader built with -fsanitize=address,undefined and run as a child process."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import ocffm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "one-class-ffm_amd", "csrc")
SAN = os.path.join(REPO, "tests", "sanitize")

# f = 3 fields: one user field, two item fields; k = 2
F, FU, FV, K = 3, 1, 2, 2
DS = [2, 3, 1]
BLOCKS = [(f1, f2) for f1 in range(F) for f2 in range(f1, F)]
CROSS = [(f1, f2) for f1, f2 in BLOCKS if f1 < FU <= f2]


def table(f1, f2, what):
    """Distinct values per (block, table, row, column)."""
    D = DS[f1 if what == "W" else f2]
    base = 100 * f1 + 10 * f2 + (0 if what == "W" else 5)
    return np.array([[base + r + 0.25 * c for c in range(K)] for r in range(D)], dtype=np.float64)


def text_lines(blocks):
    """{(f1, f2, what): [line, ...]} in file order for the given blocks."""
    out = {}
    for f1, f2 in blocks:
        for what in "WH":
            out[(f1, f2, what)] = [f"{what},{f1},{f2},{r} " + " ".join(f"{v:g}" for v in row)
                                   for r, row in enumerate(table(f1, f2, what))]
    return out


def header_lines():
    return [str(F), str(FU), str(FV), str(K)] + [str(d) for d in DS]


def text_model(blocks, edit=None):
    tabs = text_lines(blocks)
    if edit:
        edit(tabs)
    lines = header_lines()
    for rows in tabs.values():
        lines += rows
    return "\n".join(lines) + "\n"


def binary_model(blocks):
    """(bytes, boundaries): the snapshot and the offset after every section."""
    b = struct.pack("<4I", F, FU, FV, K)
    cuts = [len(b)]
    b += struct.pack(f"<{F}Q", *DS)
    cuts.append(len(b))
    for f1, f2 in blocks:
        W, H = table(f1, f2, "W"), table(f1, f2, "H")
        for part in (struct.pack("<I", ocffm.block_index(f1, f2, F)), struct.pack("<Q", W.size),
                     struct.pack("<Q", H.size), W.tobytes(), H.tobytes()):
            b += part
            cuts.append(len(b))
    return b, cuts


def put(tmp_path, name, data):
    p = tmp_path / name
    if isinstance(data, bytes):
        p.write_bytes(data)
    else:
        p.write_text(data)
    return str(p)


def code_of(path, binary):
    with pytest.raises(ocffm.OcffmError) as e:
        ocffm.model_file_info(path, binary)
    return e.value.code


def drop(key):
    return lambda tabs: tabs.pop(key)


def drop_row(key, r):
    return lambda tabs: tabs[key].pop(r)


def repeat_row(key, r):
    return lambda tabs: tabs[key].insert(r, tabs[key][r])


def swap_rows(key):
    def f(tabs):
        tabs[key][0], tabs[key][1] = tabs[key][1], tabs[key][0]
    return f


def edit_row(key, r, fn):
    def f(tabs):
        tabs[key][r] = fn(tabs[key][r])
    return f


BAD_TEXT = {
    "cross block absent": lambda t: (t.pop((0, 2, "W")), t.pop((0, 2, "H"))),
    "only W of a cross block": drop((0, 1, "H")),
    "only H of a cross block": drop((0, 1, "W")),
    "only W of a side block": drop((1, 2, "H")),
    "only H of a side block": drop((1, 1, "W")),
    "only some side blocks": lambda t: (t.pop((1, 2, "W")), t.pop((1, 2, "H"))),
    "missing row": drop_row((0, 1, "H"), 1),
    "missing last row": drop_row((0, 1, "H"), 2),
    "repeated row": repeat_row((0, 1, "W"), 1),
    "rows out of order": swap_rows((0, 1, "H")),
    "too few values": edit_row((0, 2, "W"), 0, lambda s: s.rsplit(" ", 1)[0]),
    "too many values": edit_row((0, 2, "W"), 1, lambda s: s + " 1.5"),
    "non-numeric token": edit_row((0, 1, "W"), 0, lambda s: s.rsplit(" ", 1)[0] + " abc"),
    "number with a tail": edit_row((0, 1, "W"), 0, lambda s: s + "x"),
    "non-numeric row index": edit_row((0, 1, "W"), 0, lambda s: s.replace("W,0,1,0 ", "W,0,1,zero ")),
    "bad table letter": edit_row((0, 1, "W"), 0, lambda s: "Q" + s[1:]),
}


def test_good_text_model(tmp_path):
    i = ocffm.model_file_info(put(tmp_path, "m.txt", text_model(BLOCKS)))
    assert (i["f"], i["fu"], i["fv"], i["k"], i["kp"]) == (F, FU, FV, K, 4)
    assert i["Ds"].tolist() == DS
    assert i["nblocks"] == 6 and i["nused"] == 6 and i["used"].all() and i["self_side"]
    assert not i["has_items"] and i["n"] == 0


def test_ns_text_model_has_unused_side_blocks(tmp_path):
    i = ocffm.model_file_info(put(tmp_path, "m.txt", text_model(CROSS)))
    assert i["nused"] == 2 and not i["self_side"]
    assert [b for b in range(6) if i["used"][b]] == [ocffm.block_index(f1, f2, F) for f1, f2 in CROSS]


@pytest.mark.parametrize("case", sorted(BAD_TEXT))
def test_malformed_text_model(tmp_path, case):
    assert code_of(put(tmp_path, "m.txt", text_model(BLOCKS, BAD_TEXT[case])), False) == ocffm.E_DATA


def test_text_model_header_and_tail(tmp_path):
    good = text_model(BLOCKS)
    assert code_of(put(tmp_path, "a", good + "garbage\n"), False) == ocffm.E_DATA
    assert code_of(put(tmp_path, "b", good + good.splitlines()[-1] + "\n"), False) == ocffm.E_DATA
    assert code_of(put(tmp_path, "c", good.replace("3\n1\n2\n2\n", "3\n1\n2\nx\n", 1)), False) == ocffm.E_DATA
    assert code_of(put(tmp_path, "d", good.replace("3\n1\n2\n2\n", "3\n2\n2\n2\n", 1)), False) == ocffm.E_DATA
    assert code_of(put(tmp_path, "e", good.replace("3\n1\n2\n2\n", "3\n1\n2\n129\n", 1)), False) == ocffm.E_DATA
    assert code_of(put(tmp_path, "f", "\n".join(header_lines()[:5]) + "\n"), False) == ocffm.E_DATA
    assert code_of(put(tmp_path, "g", ""), False) == ocffm.E_DATA
    assert code_of(str(tmp_path / "nope"), False) == ocffm.E_IO


def test_good_binary_model(tmp_path):
    for blocks, nused in ((BLOCKS, 6), (CROSS, 2)):
        i = ocffm.model_file_info(put(tmp_path, "m.bin", binary_model(blocks)[0]), binary=True)
        assert (i["f"], i["fu"], i["fv"], i["k"]) == (F, FU, FV, K)
        assert i["Ds"].tolist() == DS and i["nused"] == nused and i["self_side"] == (nused == 6)


@pytest.mark.parametrize("blocks", [BLOCKS, CROSS], ids=["all", "ns"])
def test_truncated_binary_model(tmp_path, blocks):
    data, cuts = binary_model(blocks)
    assert cuts[-1] == len(data)
    for c in cuts[:-1]:  # at every section boundary, and inside the section before it
        for n in (c, c - 1):
            assert code_of(put(tmp_path, "m.bin", data[:n]), True) == ocffm.E_DATA, n
    assert code_of(put(tmp_path, "m.bin", data[:-1]), True) == ocffm.E_DATA
    assert code_of(put(tmp_path, "m.bin", b""), True) == ocffm.E_DATA


def test_malformed_binary_model(tmp_path):
    data, cuts = binary_model(BLOCKS)
    assert code_of(put(tmp_path, "a", data + b"\0"), True) == ocffm.E_DATA  # trailing bytes
    assert code_of(put(tmp_path, "b", data + data[cuts[1]:]), True) == ocffm.E_DATA  # the blocks twice
    wrong_idx = bytearray(data)
    wrong_idx[cuts[1]:cuts[1] + 4] = struct.pack("<I", 4)
    assert code_of(put(tmp_path, "c", bytes(wrong_idx)), True) == ocffm.E_DATA
    wrong_size = bytearray(data)
    wrong_size[cuts[2]:cuts[2] + 8] = struct.pack("<Q", DS[0] * K + 1)
    assert code_of(put(tmp_path, "d", bytes(wrong_size)), True) == ocffm.E_DATA
    huge = bytearray(data)
    huge[0:4] = struct.pack("<I", 0xFFFFFFFF)  # a field count from garbage
    assert code_of(put(tmp_path, "e", bytes(huge)), True) == ocffm.E_DATA
    some = binary_model(BLOCKS[:-1])[0]  # the last side block missing
    assert code_of(put(tmp_path, "f", some), True) == ocffm.E_DATA
    assert code_of(str(tmp_path / "nope"), True) == ocffm.E_IO
    # a text model read as a snapshot and the reverse
    assert code_of(put(tmp_path, "g", text_model(BLOCKS)), True) == ocffm.E_DATA
    assert code_of(put(tmp_path, "h", data), False) == ocffm.E_DATA


def test_every_model_symbol_is_exported():
    lib = ocffm.lib()
    header = open(os.path.join(REPO, "include", "ocffm.h")).read()
    syms = sorted(set(re.findall(r"\b(ocffm_model_[a-z_0-9]+)\s*\(", header)))
    assert len(syms) == 18
    for s in syms:
        assert s in ocffm.EXPORTS and hasattr(lib, s), s
    for name in ("Model", "model_file_info"):
        assert hasattr(ocffm, name)


def test_reader_under_sanitizers(tmp_path):
    """The reader's source with a stand-alone driver (tests/sanitize/
    model_file_driver.cpp), built with ASan + UBSan and run as a child process
    on the good and malformed files above: the statuses are those of the
    library, and no sanitizer report (a report aborts: non-zero exit)."""
    out_dir = os.path.join(SAN, "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "model_file_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-Wall", "-I" + CSRC, "-o", exe,
                    os.path.join(SAN, "model_file_driver.cpp"), os.path.join(CSRC, "model_file.cpp")], check=True)
    data, cuts = binary_model(BLOCKS)
    files = [("t", put(tmp_path, "good.txt", text_model(BLOCKS)), 0), ("t", put(tmp_path, "ns.txt", text_model(CROSS)), 0),
             ("b", put(tmp_path, "good.bin", data), 0), ("b", put(tmp_path, "ns.bin", binary_model(CROSS)[0]), 0),
             ("t", str(tmp_path / "nope"), ocffm.E_IO), ("b", put(tmp_path, "tail.bin", data + b"\0"), ocffm.E_DATA),
             ("t", put(tmp_path, "as_text.txt", data), ocffm.E_DATA),
             ("b", put(tmp_path, "as_bin.bin", text_model(BLOCKS)), ocffm.E_DATA)]
    for q, case in enumerate(sorted(BAD_TEXT)):
        files.append(("t", put(tmp_path, f"bad{q}.txt", text_model(BLOCKS, BAD_TEXT[case])), ocffm.E_DATA))
    for q, c in enumerate(cuts[:-1]):
        files.append(("b", put(tmp_path, f"cut{q}.bin", data[:c]), ocffm.E_DATA))
        files.append(("b", put(tmp_path, f"cutm{q}.bin", data[:c - 1]), ocffm.E_DATA))
    argv = [exe]
    for mode, path, _ in files:
        argv += [mode, path]
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:exitcode=99:detect_leaks=1",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run(argv, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(files)
    for (mode, path, want), line in zip(files, lines):
        assert int(line.split()[0]) == want, (path, line)
    assert lines[0] == "0 3 1 2 2 4 6 1 | 2 3 1 | 1 1 1 1 1 1"
    assert lines[1] == "0 3 1 2 2 4 2 0 | 2 3 1 | 0 1 1 0 0 0"
    assert lines[2] == lines[0] and lines[3] == lines[1]

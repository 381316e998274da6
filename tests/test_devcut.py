"""The device block cut's logic (fastqueeze_amd/csrc/sa_devcut.h: what k_dt_count
and k_dt_cut run) on the CPU: tests/cpu_emu/devcut_emu.cpp drives it with the
wave's lanes as a loop over a host stand-in for sa_devtext's buffer, and checks
every block length and every reason a cut stopped against sa_cut_next_se /
sa_cut_next_pe of fastq_host.cpp on the same bytes.  Built plainly and with
-fsanitize=address,undefined; the kernels run on the device only after this
(tests/test_gpu_devtext.py)."""
import os
import subprocess

import pytest

import devcut_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tests", "cpu_emu", "devcut_emu.cpp"), os.path.join(ROOT, "fastqueeze_amd", "csrc", "fastq_host.cpp")]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("devcut_emu")
    exe, san = d / "devcut_emu", d / "devcut_emu_san"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", "-o", str(exe)] + SRC, check=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(san)] + SRC, check=True)
    return exe, san


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("devcut_in")
    out = {}
    for tag, (a, b) in (("synth", dc.synth_pair()), ("golden", dc.golden_pair())):
        p1, p2 = d / f"{tag}_1.fq", d / f"{tag}_2.fq"
        p1.write_bytes(a)
        p2.write_bytes(b)
        out[tag] = (str(p1), str(p2))
    return out


def run(exe, f1, f2, bs, piece=0, cap=0, max_blocks=64, eof=True, nocarry=False):
    """(blocks, end, nocarry blocks or None, moves): the emulation's answer; it
    exits non-zero itself when the device logic and the host cut differ."""
    cmd = [str(exe), f1, f2 or "-", str(bs), str(piece), str(cap), str(max_blocks), "1" if eof else "0"]
    r = subprocess.run(cmd + (["nocarry"] if nocarry else []), capture_output=True, text=True)
    assert r.returncode == 0, (cmd, r.stdout[-400:], r.stderr[-2000:])
    blocks, alt, last = [], [], None
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "B":
            blocks.append((int(w[1]), int(w[2])))
        elif w[0] == "NOCARRY" and w[1] == "B":
            alt.append((int(w[2]), int(w[3])))
        elif w[0] == "end":
            last = w
    assert last is not None and int(last[3]) == len(blocks)
    return blocks, int(last[1]), (alt if nocarry else None), int(last[5])


COUNTS = {("synth", True): dc.SYNTH_PE, ("synth", False): dc.SYNTH_SE, ("golden", True): dc.GOLDEN_PE}


@pytest.mark.parametrize("which,pe", [("synth", True), ("synth", False), ("golden", True)])
@pytest.mark.parametrize("bi", range(len(dc.BLOCK_SIZES)))
def test_whole_and_pieces(emu, files, which, pe, bi):
    """Whole input in one buffer, and the same input in 300,001-byte pieces
    through a 3 MiB buffer (cut and take after each piece: 'more', the move to
    the front, read positions off the tile grid): every block as the host cuts
    it, none left out, the pieces' blocks the whole buffer's."""
    f1, f2 = files[which]
    bs = dc.BLOCK_SIZES[bi]
    whole, end, _, moves = run(emu[0], f1, f2 if pe else None, bs)
    assert end == dc.DONE and moves == 0
    assert len(whole) == COUNTS[(which, pe)][bi]
    size = os.path.getsize(f1), os.path.getsize(f2)
    assert sum(b[0] for b in whole) == size[0] and (not pe or sum(b[1] for b in whole) == size[1])
    parts, end, _, moves = run(emu[0], f1, f2 if pe else None, bs, piece=dc.PIECE, cap=dc.PIECE_CAP, max_blocks=7)
    assert end == dc.DONE and parts == whole
    assert moves > 0 or size[0] <= dc.PIECE_CAP


def test_sanitized_pieces(emu, files):
    """The sanitizer build over the paths above at the sizes that take them all."""
    f1, f2 = files["golden"]
    for bs in (8192, 65537):
        run(emu[1], f1, f2, bs)
        run(emu[1], f1, f2, bs, piece=dc.PIECE, cap=dc.PIECE_CAP, max_blocks=7)
        run(emu[1], f1, None, bs, piece=dc.PIECE, cap=dc.PIECE_CAP, max_blocks=7)
    g1, g2 = files["synth"]
    run(emu[1], g1, g2, 3000001, piece=dc.PIECE, cap=dc.PIECE_CAP)


@pytest.mark.parametrize("case", dc.cases(), ids=lambda c: c["name"])
def test_hand_built(emu, tmp_path, case):
    """The hand-built cases, plain and under the sanitizers, whole and in
    97-byte pieces through a small buffer."""
    p1, p2 = tmp_path / "a.fq", tmp_path / "b.fq"
    p1.write_bytes(case["t1"])
    if case["t2"] is not None:
        p2.write_bytes(case["t2"])
    f2 = str(p2) if case["t2"] is not None else None
    got = None
    for exe in emu:
        if case["end"] == dc.FULL:
            blocks, end, alt, _ = _one_call(exe, str(p1), f2, case)
        else:
            blocks, end, alt, _ = run(exe, str(p1), f2, case["bs"], eof=case["eof"], nocarry=case["nocarry_differs"])
        assert got is None or got == (blocks, end, alt)
        got = (blocks, end, alt)
        if case["end"] is not None:
            assert end == case["end"], (case["name"], end)
        if case["blocks"] is not None:
            assert len(blocks) == case["blocks"], (case["name"], blocks)
        if case["nocarry_differs"]:
            assert alt != blocks, "a counter reset at every candidate gives the same cut: the case shows nothing"
        cap = max(8192, 2 * case["bs"])
        if case["end"] != dc.FULL and max(len(case["t1"]), len(case["t2"] or b"")) > 97:
            parts, pend, _, _ = run(exe, str(p1), f2, case["bs"], piece=97, cap=cap, max_blocks=5, eof=case["eof"])
            if case["eof"]:
                assert (parts, pend) == (blocks, end), case["name"]


def _one_call(exe, f1, f2, case):
    """A case that ends with 'full': the first cut call's blocks only."""
    cmd = [str(exe), f1, f2 or "-", str(case["bs"]), "0", "0", str(case["max_blocks"]), "1" if case["eof"] else "0"]
    r = subprocess.run(cmd + (["nocarry"] if case["nocarry_differs"] else []), capture_output=True, text=True)
    assert r.returncode == 0, (cmd, r.stderr[-2000:])
    blocks, alt, end = [], [], None
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "E":
            end = int(w[1])
            break
        if w[0] == "B":
            blocks.append((int(w[1]), int(w[2])))
        elif w[0] == "NOCARRY" and w[1] == "B":
            alt.append((int(w[2]), int(w[3])))
    return blocks, end, (alt if case["nocarry_differs"] else None), 0

"""CPU: csrc/jpeg_parse.cpp and the per-interval decoder body of csrc/jpeg_dec_dev.hpp as a stand-alone host program
(tests/jpeg_dec_check.cpp) under the address and undefined-behaviour sanitizers, on every case stream, every prefix
of each and 2,000 seeded single-byte mutations of each: no sanitizer report, and parse code, status and coefficients
equal to the restatement's (tests/jpeg_dec_ref.py) on every input."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_dec_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "macaque-3d-pose-estimation_amd", "csrc")
N_MUTATIONS = 2000


def _compilers():
    for c in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++"):
        if c and shutil.which(c):
            yield shutil.which(c)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """(path, sanitized): the check program with -fsanitize=address,undefined, the sanitizer runtime linked
    statically so that the program starts in any environment; unsanitised if no compiler here builds one that starts."""
    tmp = tmp_path_factory.mktemp("jpeg_dec_check")
    out, empty = str(tmp / "jpeg_dec_check"), str(tmp / "empty.bin")
    open(empty, "wb").close()
    src = [os.path.join(ROOT, "tests", "jpeg_dec_check.cpp"), os.path.join(CSRC, "jpeg_parse.cpp")]
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    errors = []
    for flags in (san + ["-static-libsan"], san + ["-static-libasan", "-static-libubsan"], san, []):
        for cxx in _compilers():
            r = subprocess.run([cxx, "-std=c++17", "-O1", "-Werror", *flags, *inc, *src, "-o", out],
                               capture_output=True, text=True)
            if r.returncode == 0:
                r = subprocess.run([out, empty], capture_output=True, text=True)
                if r.returncode == 0 and not r.stderr.strip():
                    return out, bool(flags)
            errors.append(f"{cxx} {flags}: {r.stderr[-300:]}")
    pytest.fail("no host compiler built a tests/jpeg_dec_check.cpp that starts:\n" + "\n".join(errors))


def _run(program, tmp_path, inputs):
    path = str(tmp_path / "records.bin")
    with open(path, "wb") as f:
        for d in inputs:
            f.write(struct.pack("<I", len(d)) + d)
    r = subprocess.run([program[0], path], capture_output=True, text=True)      # the environment as it is
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-2000:])
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(inputs)
    return [tuple(ln.split()) for ln in lines]


def _expect(d):
    """What the program prints for ``d``, from the restatement."""
    try:
        info = D.parse(d)
    except D.ParseError as e:
        return (str(e.code), "-1", "0" * 16, "0")
    n_mcu = info.mcus[0] * info.mcus[1]
    if n_mcu * info.blocks > 65536:
        return ("0", "-2", "0" * 16, "0")
    coef = np.zeros((n_mcu, info.blocks, 64), dtype=np.int64)
    stats = {}
    st = D.decode_status(d, info, stats, coef)
    if st == D.ST_MARKERS:
        return ("0", "1", "0" * 16, "0")
    c = coef.reshape(-1).astype(np.int16).astype(np.uint16).astype(np.uint64)
    h = int((c * (2 * np.arange(len(c), dtype=np.uint64) + 1)).sum(dtype=np.uint64))
    return ("0", str(st), f"{h:016x}", str(stats.get("long_codes", 0)))


def _check(program, tmp_path, inputs):
    got = _run(program, tmp_path, inputs)
    for i, (d, g) in enumerate(zip(inputs, got)):
        assert g == _expect(d), (i, len(d), g, _expect(d))
    return got


def test_the_program_is_sanitized(program):
    """If no compiler here builds a sanitized program that starts, the other tests still run it, unsanitised: this
    test says so."""
    assert program[1], "built without -fsanitize=address,undefined"


def test_valid_streams(program, tmp_path):
    cases = D.case_streams()
    got = _check(program, tmp_path, list(cases.values()) + [d for _, d in D.pillow_streams()])
    assert all(g[:2] == ("0", "0") for g in got)
    assert int(got[list(cases).index("40x56-420opt")][3]) > 0          # the walk past the first-level lookup ran


@pytest.mark.parametrize("name", list(D.case_streams()))
def test_every_prefix(program, tmp_path, name):
    d = D.case_streams()[name]
    got = _check(program, tmp_path, [d[:k] for k in range(len(d))])
    assert all(g[0] != "0" for g in got[:len(d) - 2])                  # no EOI yet: refused


@pytest.mark.parametrize("name", list(D.case_streams()))
def test_seeded_single_byte_mutations(program, tmp_path, name):
    d = D.case_streams()[name]
    rng = np.random.default_rng(sum(name.encode()))
    inputs = []
    for _ in range(N_MUTATIONS):
        m = bytearray(d)
        m[int(rng.integers(len(d)))] = int(rng.integers(256))
        inputs.append(bytes(m))
    got = _check(program, tmp_path, inputs)
    kinds = {g[:2] for g in got}
    print(name, sorted(kinds))
    assert len(kinds) >= 2


def test_idct_wrap_rule_never_triggers_on_a_valid_stream():
    for name, d in list(D.case_streams().items()) + D.pillow_streams():
        stats = {}
        _, st = D.decode(d, stats=stats)
        assert st == 0 and not stats.get("wrapped"), name

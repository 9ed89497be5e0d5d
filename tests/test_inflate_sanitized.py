"""The wave's inflate under AddressSanitizer and UBSan: ``tests/native/inflate_sanitized.cpp`` -- csrc/gsr_inflate_core.h and a
``main``, nothing else of the project -- built here with the host C++ compiler and run as a child process on the hand-made corpora
(``deflate_streams``: A ... D), the zlib corpus and every 50th stream of the seek corpus.  Every buffer it passes is a heap block of
exactly the contract's size, so a byte read or written outside one ends the process with a report.  CPU only."""
import os
import shutil
import struct
import subprocess
import time
import zlib

import pytest

import deflate_streams as ds
from test_layer_io import _host_lane_inflate, _zlib_corpus, _zlib_seek_corpus

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "autovfx_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
MUTATIONS_PER_STREAM = 20
MUTATION_SEED = 0x9E3779B97F4A7C15


def _compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    tmp = tmp_path_factory.mktemp("inflate_sanitized")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked into the program where the compiler can (then the program does not care what else a machine loads into
    # every process in front of it), else the shared ones
    for flags in (FLAGS + ["-static-libasan", "-static-libubsan"], FLAGS):
        linked = subprocess.run([cxx, *flags, str(probe), "-o", str(tmp / "probe")], capture_output=True, text=True)
        if linked.returncode == 0:
            break
    else:
        pytest.skip(f"{cxx} cannot link a sanitized program: {linked.stderr.strip()[-200:]}")
    exe = tmp / "inflate_sanitized"
    subprocess.run([cxx, *flags, "-I", CSRC, os.path.join(HERE, "native", "inflate_sanitized.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def sanitized_corpus():
    """``[(name, stream, expected bytes)]``: what the sanitized program runs -- and the only streams the GPU test of the refused streams
    may launch (it takes its list from here)."""
    out = [(name, stream, len(data)) for name, stream, data in ds.good_corpora()]
    out += [(name, stream, n) for name, stream, n, _status in ds.corpus_d()]
    out += [(f"zlib corpus {k}", stream, len(data)) for k, (stream, data) in enumerate(_zlib_corpus())]
    out += [(f"seek corpus {50 * k}", stream, len(data)) for k, (stream, data) in enumerate(_zlib_seek_corpus()[::50])]
    return out


@pytest.fixture(scope="module")
def container(tmp_path_factory):
    corpus = sanitized_corpus()
    path = tmp_path_factory.mktemp("inflate_corpus") / "streams.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(corpus)))
        for _name, stream, n in corpus:
            f.write(struct.pack("<II", len(stream), n) + stream)
    return str(path), corpus


def _run(argv):
    t0 = time.perf_counter()
    done = subprocess.run(argv, capture_output=True, text=True, timeout=600)
    return done, time.perf_counter() - t0


def test_sanitized_host_lane_is_the_library(program, container):
    """Every stream of the corpus through the sanitized build: exit status 0, nothing on stderr, and status and output (its Adler-32)
    equal to what the library's host lane returns in this process -- the sanitized build is the same code, and it ran clean."""
    path, corpus = container
    done, seconds = _run([program, path])
    print(f"sanitized run: {len(corpus)} streams in {seconds:.1f} s")
    assert done.returncode == 0 and done.stderr == "", done.stderr[-3000:]
    lines = done.stdout.splitlines()
    assert len(lines) == len(corpus)
    bad = []
    for k, (name, stream, n) in enumerate(corpus):
        rc, out = _host_lane_inflate(stream, n)
        if lines[k] != f"{k} {rc} {zlib.adler32(out):08x}":
            bad.append((name, lines[k], rc))
    assert not bad, f"{len(bad)} streams differ (name, the program's line, the library's status): {bad[:10]}"


def test_sanitized_host_lane_survives_damaged_streams(program, container):
    """Mutation mode: per corpus stream N = 20 variants -- a bit flipped, a byte replaced, the tail cut, the output size off by 1 ... 300,
    two streams spliced -- seeded; asserted is only that the process finishes with exit status 0 and an empty stderr, i.e. that no
    variant made the decoder touch a byte outside its buffers.  (2 568 streams, 51 360 variants: 12 s of the module's 20 s on the machine this was sized on.)"""
    path, corpus = container
    done, seconds = _run([program, path, "--mutate", str(MUTATION_SEED), str(MUTATIONS_PER_STREAM)])
    print(f"mutation run: {len(corpus)} streams, N = {MUTATIONS_PER_STREAM} variants each, {seconds:.1f} s: {done.stdout.strip()}")
    assert done.returncode == 0 and done.stderr == "", done.stderr[-3000:]
    assert done.stdout.startswith(f"mutations {MUTATIONS_PER_STREAM * len(corpus)} ")

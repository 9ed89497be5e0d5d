"""The wave64 scan of gsr_wave.h (wave_scan_steps: four row shifts, two row broadcasts) without a kernel: the SAME steps,
instantiated over a 64-lane host model of the DPP moves (a lane without a source, or in a row the row mask leaves out, gets
zero), against a serial scan.  Patterns: for each of the values 1 and 0xFFFF every prefix of the wave (lanes below k hold the
value, the others zero: k = 0 .. 64), the complements of those prefixes, and random words that wrap around 2^32.  The 64-bit
instantiation (the mesh rasterizer's scan) runs the same patterns, with the value 0xFFFFFFFF added, whose sums carry into the
high word, and random words that wrap around 2^64.  The program counts its cases and fails on a count it does not expect."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "gsr_wave.h"
#include <cstdio>
#include <cstdint>

template <class T>
struct Lanes {
    T l[64];
    Lanes operator+(const Lanes& o) const { Lanes r; for (int i = 0; i < 64; ++i) r.l[i] = l[i] + o.l[i]; return r; }
};

// dpp_ctrl as the ISA defines it: row_shr:n moves lane i - n of the SAME row of 16 to lane i; row_bcast:15 moves lane 15 of each
// row to every lane of the next row; row_bcast:31 moves lane 31 to every lane of rows 2 and 3.
struct ModelMoves {
    template <int kCtrl, int kRowMask, class T>
    static Lanes<T> moved(const Lanes<T>& v) {
        Lanes<T> r;
        for (int i = 0; i < 64; ++i) {
            const int row = i / 16;
            int src = -1;
            if (kCtrl > gsr::kDppRowShr && kCtrl < gsr::kDppRowShr + 16) { if (i % 16 >= kCtrl - gsr::kDppRowShr) src = i - (kCtrl - gsr::kDppRowShr); }
            else if (kCtrl == gsr::kDppRowBcast15) { if (row >= 1) src = 16 * row - 1; }
            else if (kCtrl == gsr::kDppRowBcast31) { if (row >= 2) src = 31; }
            r.l[i] = (src >= 0 && ((kRowMask >> row) & 1)) ? v.l[src] : T(0);
        }
        return r;
    }
};

template <class T>
static int check(const Lanes<T>& v, const char* what, int k) {
    const Lanes<T> got = gsr::wave_scan_steps<ModelMoves>(v);
    T sum = 0;
    for (int i = 0; i < 64; ++i) {
        sum += v.l[i];
        if (got.l[i] != sum) {
            std::printf("%s %d: lane %d holds %llu, serial scan %llu\n", what, k, i, (unsigned long long)got.l[i], (unsigned long long)sum);
            return 1;
        }
    }
    return 0;
}

// every prefix and suffix of the wave for each value, then 200 waves of random words: *cases counts them
template <class T, int kValues>
static int run(const T (&values)[kValues], int* cases) {
    int bad = 0;
    for (T value : values)
        for (int k = 0; k <= 64; ++k) {
            Lanes<T> a, b;
            for (int i = 0; i < 64; ++i) { a.l[i] = i < k ? value : T(0); b.l[i] = i < k ? T(0) : value; }
            bad += check(a, "prefix", k) + check(b, "suffix", k);
            *cases += 2;
        }
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (int k = 0; k < 200; ++k) {
        Lanes<T> a;
        for (int i = 0; i < 64; ++i) { s = s * 6364136223846793005ull + 1442695040888963407ull; a.l[i] = (T)(sizeof(T) == 8 ? s : s >> 32); }
        bad += check(a, "random", k);
        ++*cases;
    }
    return bad;
}

int main() {
    int cases = 0, cases64 = 0;
    const uint32_t values[2] = {1u, 0xFFFFu};
    const int bad = run(values, &cases);
    std::printf("%d cases, %d wrong\n", cases, bad);
    const unsigned long long values64[3] = {1ull, 0xFFFFull, 0xFFFFFFFFull};
    const int bad64 = run(values64, &cases64);
    std::printf("%d cases of 64 bits, %d wrong\n", cases64, bad64);
    if (cases != 2 * 65 * 2 + 200 || cases64 != 3 * 65 * 2 + 200) { std::printf("unexpected case count\n"); return 2; }
    return bad != 0 || bad64 != 0;
}
"""


def test_scan_steps_on_a_host_model_of_the_lane_moves(tmp_path):
    from autovfx_amd import build
    cc = build.hipcc()
    src, exe = tmp_path / "wave_scan_host.hip", tmp_path / "wave_scan_host"
    src.write_text(PROGRAM)
    subprocess.check_call([cc, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-I", build.CSRC, "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "460 cases, 0 wrong" in out.stdout
    assert "590 cases of 64 bits, 0 wrong" in out.stdout

"""The wave64 scan of gsr_device.h (wave_scan_steps: four row shifts, two row broadcasts) without a kernel: the SAME steps,
instantiated over a 64-lane host model of the DPP moves (a lane without a source, or in a row the row mask leaves out, gets
zero), against a serial scan.  Patterns: for each of the values 1 and 0xFFFF every prefix of the wave (lanes below k hold the
value, the others zero: k = 0 .. 64), the complements of those prefixes, and random words that wrap around 2^32."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "gsr_device.h"
#include <cstdio>
#include <cstdint>

struct Lanes {
    uint32_t l[64];
    Lanes operator+(const Lanes& o) const { Lanes r; for (int i = 0; i < 64; ++i) r.l[i] = l[i] + o.l[i]; return r; }
};

// dpp_ctrl as the ISA defines it: row_shr:n moves lane i - n of the SAME row of 16 to lane i; row_bcast:15 moves lane 15 of each
// row to every lane of the next row; row_bcast:31 moves lane 31 to every lane of rows 2 and 3.
struct ModelMoves {
    template <int kCtrl, int kRowMask>
    static Lanes moved(const Lanes& v) {
        Lanes r;
        for (int i = 0; i < 64; ++i) {
            const int row = i / 16;
            int src = -1;
            if (kCtrl > gsr::kDppRowShr && kCtrl < gsr::kDppRowShr + 16) { if (i % 16 >= kCtrl - gsr::kDppRowShr) src = i - (kCtrl - gsr::kDppRowShr); }
            else if (kCtrl == gsr::kDppRowBcast15) { if (row >= 1) src = 16 * row - 1; }
            else if (kCtrl == gsr::kDppRowBcast31) { if (row >= 2) src = 31; }
            r.l[i] = (src >= 0 && ((kRowMask >> row) & 1)) ? v.l[src] : 0u;
        }
        return r;
    }
};

static int check(const Lanes& v, const char* what, int k) {
    const Lanes got = gsr::wave_scan_steps<ModelMoves>(v);
    uint32_t sum = 0;
    for (int i = 0; i < 64; ++i) {
        sum += v.l[i];
        if (got.l[i] != sum) { std::printf("%s %d: lane %d holds %u, serial scan %u\n", what, k, i, got.l[i], sum); return 1; }
    }
    return 0;
}

int main() {
    int bad = 0, cases = 0;
    const uint32_t values[2] = {1u, 0xFFFFu};
    for (uint32_t value : values)
        for (int k = 0; k <= 64; ++k) {
            Lanes a, b;
            for (int i = 0; i < 64; ++i) { a.l[i] = i < k ? value : 0u; b.l[i] = i < k ? 0u : value; }
            bad += check(a, "prefix", k) + check(b, "suffix", k);
            cases += 2;
        }
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (int k = 0; k < 200; ++k) {
        Lanes a;
        for (int i = 0; i < 64; ++i) { s = s * 6364136223846793005ull + 1442695040888963407ull; a.l[i] = (uint32_t)(s >> 32); }
        bad += check(a, "random", k);
        ++cases;
    }
    std::printf("%d cases, %d wrong\n", cases, bad);
    return bad != 0;
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

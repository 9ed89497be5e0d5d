"""The quadrant blend's `power` with its per-column and per-row terms taken out of the per-pixel walk (gsr_device.h:
``blend_power_terms`` / ``blend_power``; gsr_blend.hip stages the terms once per entry and the walk finishes a pixel with an add, a
multiply and a subtract), without a GPU:

  * a host program evaluates the helpers for all 64 pixels of a quadrant against the expression of the walk they replace, written
    out step by step -- the same operations on the same operands, unfused, so the same 32 bits wherever the result is finite.  Two
    NaNs count as equal here whatever their sign and payload: which operand's NaN an addition returns is the host compiler's
    choice; on the device tests/test_blend_terms_gpu.py compares the bits;
  * the kernel descriptors of the cross-compiled unit: no scratch, at most 64 vector registers (eight waves per SIMD), and LDS that
    lets 32 single-wave workgroups share a CU's 160 KiB;
  * the instruction census of the walk: at most 6 vector instructions from the start of an entry's evaluation to its first early
    exit, averaged over the unrolled body (13 before the terms were taken out).
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "gsr_device.h"
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <limits>

using namespace gsr;

static uint64_t s = 0x9E3779B97F4A7C15ull;
static float rnd() {   // uniform in [-1, 1)
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((double)(s >> 11) / 9007199254740992.0 * 2.0 - 1.0);
}
static bool same(float a, float b) {
    if (a != a && b != b) return true;
    return std::memcmp(&a, &b, 4) == 0;
}

struct Entry { float x, y, mh_cxx, cxy, mh_cyy; };

// the walk's expression before the terms were taken out, one rounding per line
static float power_of(const Entry& e, int px, int py) {
    const float fx = (float)px, fy = (float)py;
    const float dx = e.x - fx;
    const float dy = e.y - fy;
    const float ax = e.mh_cxx * dx;
    const float a = ax * dx;
    const float cy = e.mh_cyy * dy;
    const float c = cy * dy;
    const float sum = a + c;
    const float bx = e.cxy * dx;
    const float b = bx * dy;
    return sum - b;
}

static const int kOrigins[5][2] = {{0, 0}, {8, 0}, {0, 8}, {1912, 1072}, {65520, 65520}};
static long pixels = 0;

static int check(const Entry& e, const char* what, int k) {
    int bad = 0;
    for (const auto& o : kOrigins) {
        float2 col[8], row[8];
        blend_power_terms(e.x, e.y, e.mh_cxx, e.cxy, e.mh_cyy, o[0], o[1], col, row);
        for (int lane = 0; lane < 64; ++lane) {
            const float got = blend_power(col[lane & 7], row[lane >> 3]);
            const float want = power_of(e, o[0] + (lane & 7), o[1] + (lane >> 3));
            ++pixels;
            if (same(got, want)) continue;
            if (bad++ == 0) std::printf("%s %d, origin (%d, %d), lane %d: %a against %a\n", what, k, o[0], o[1], lane, got, want);
        }
    }
    return bad != 0;
}

// a centre near (or, `far`: up to 1e4 pixels outside) one of the quadrants, a conic of the given magnitude
static Entry random_entry(int k, float far, float magnitude) {
    const int* o = kOrigins[k % 5];
    Entry e;
    e.x = (float)o[0] + 4.0f + rnd() * (6.0f + far);
    e.y = (float)o[1] + 4.0f + rnd() * (6.0f + far);
    e.mh_cxx = -0.5f * (0.001f + 0.5f * (rnd() + 1.0f)) * magnitude;
    e.mh_cyy = -0.5f * (0.001f + 0.5f * (rnd() + 1.0f)) * magnitude;
    e.cxy = 0.7f * rnd() * magnitude;
    return e;
}

int main() {
    int bad = 0, cases = 0;
    for (int k = 0; k < 2000; ++k) {                       // random conics and centres, every fourth 1e4 pixels outside
        bad += check(random_entry(k, k % 4 == 0 ? 1.0e4f : 0.0f, k % 7 == 0 ? 30.0f : 1.0f), "random", k);
        ++cases;
    }
    for (int k = 0; k < 500; ++k) {                        // sub-pixel centres: a centre within 1e-3 of a pixel centre
        Entry e = random_entry(k, 0.0f, 1.0f);
        e.x = std::floor(e.x) + 1.0e-3f * rnd();
        e.y = std::floor(e.y) + 1.0e-3f * rnd();
        bad += check(e, "sub-pixel", k);
        ++cases;
    }
    for (int k = 0; k < 200; ++k) {                        // conics of 1e-38 (products go subnormal) and of 1e30 (they overflow)
        bad += check(random_entry(k, 0.0f, 1.0e-38f), "tiny conic", k);
        bad += check(random_entry(k, k % 2 ? 1.0e4f : 0.0f, 1.0e30f), "huge conic", k);
        cases += 2;
    }
    const float special[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                              -std::numeric_limits<float>::infinity()};
    for (int f = 0; f < 5; ++f)                            // every field in turn NaN, +inf, -inf
        for (float v : special)
            for (int k = 0; k < 5; ++k) {
                Entry e = random_entry(k, 0.0f, 1.0f);
                (&e.x)[f] = v;
                bad += check(e, "special", 3 * f + k);
                ++cases;
            }
    std::printf("%d cases, %ld pixels, %d wrong\n", cases, pixels, bad);
    return bad != 0;
}
"""


def test_power_from_column_and_row_terms_against_the_walk_expression_on_the_host(tmp_path):
    from autovfx_amd import build
    cc = build.hipcc()
    src, exe = tmp_path / "blend_terms_host.hip", tmp_path / "blend_terms_host"
    src.write_text(PROGRAM)
    subprocess.check_call([cc, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-I", build.CSRC,
                           "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "2975 cases, 952000 pixels, 0 wrong" in out.stdout, out.stdout[-500:]


def _scripts(name):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        return __import__(name)
    finally:
        sys.path.pop(0)


def test_blend_kernels_keep_eight_waves_per_simd():
    """Eight single-wave workgroups per SIMD, 32 per CU: 512 vector registers / 8 = 64 each, 160 KiB / 32 = 5 120 bytes of LDS
    each, nothing spilled.  (Capping the blend at six waves cost 20 %: docs/history.md, round 2.)"""
    census = _scripts("kernel_isa_census")
    from autovfx_amd import build
    asm = census.assembly(build.CSRC, "gsr_blend.hip")
    for part in ("blend_quadrant_kernelILb0", "blend_quadrant_kernelILb1"):
        c = census.census(asm, part)
        print(part, {k: c[k] for k in ("vgpr", "sgpr", "lds_bytes", "scratch")})
        assert c["scratch"] == 0, f"{part} spills {c['scratch']} bytes per lane"
        assert 0 < c["vgpr"] <= 64, f"{part} needs {c['vgpr']} vector registers: fewer than eight waves per SIMD"
        assert 0 < c["lds_bytes"] and 32 * c["lds_bytes"] <= 160 * 1024, f"{part}'s {c['lds_bytes']} bytes of LDS: fewer than 32 workgroups per CU"


def test_walk_spends_at_most_six_vector_instructions_before_the_first_early_exit():
    census = _scripts("blend_isa_census")
    for part in ("blend_quadrant_kernelILb0", "blend_quadrant_kernelILb1"):
        entries, rows = census.stage_table(part)
        print(part, entries, "entries in the body; stage A per entry:", rows[0])
        assert entries >= 1
        assert rows[0]["VALU total"] <= 6.0, f"{part}: {rows[0]['VALU total']} vector instructions per entry before the first early exit"

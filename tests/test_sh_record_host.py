"""The record-first SH evaluation of gsr_device.h (``sh_unclamped_record`` / ``sh_to_rgb_record``: sixteen coefficients already in
registers) against the coefficient-by-coefficient one (``sh_unclamped`` / ``sh_to_rgb`` at degree 3) on the host, without a kernel:
the same operations in the same order, so the same bits -- for random records and directions, for NaN and +-inf in every single
coefficient, and for a Gaussian at the camera position (a direction of 0 / 0).  Two NaNs count as equal here whatever their sign
and payload: which operand's NaN an addition returns is the host compiler's choice; on the device tests/test_sh_record_loads_gpu.py
compares the bits."""
import os
import subprocess

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
static int check(const float* sh, F3 pos, F3 cam, const char* what, int k) {
    alignas(16) float rec[48];
    std::memcpy(rec, sh, sizeof rec);
    const ShRecord r = ld_sh_record(rec);
    const F3 a = sh_to_rgb(3, pos, cam, sh), b = sh_to_rgb_record(pos, cam, r);
    const float dx = pos.x - cam.x, dy = pos.y - cam.y, dz = pos.z - cam.z, len = std::sqrt(dx * dx + dy * dy + dz * dz);
    const F3 c = sh_unclamped(3, dx / len, dy / len, dz / len, sh), d = sh_unclamped_record(dx / len, dy / len, dz / len, r);
    if (same(a.x, b.x) && same(a.y, b.y) && same(a.z, b.z) && same(c.x, d.x) && same(c.y, d.y) && same(c.z, d.z)) return 0;
    std::printf("%s %d: (%a %a %a) against (%a %a %a)\n", what, k, b.x, b.y, b.z, a.x, a.y, a.z);
    return 1;
}

int main() {
    int bad = 0, cases = 0;
    float sh[48];
    const F3 cam = {0.25f, -0.5f, -4.0f};
    for (int k = 0; k < 2000; ++k) {
        for (float& v : sh) v = rnd() * (k % 7 == 0 ? 30.0f : 1.0f);
        const F3 pos = {rnd() * 3.0f, rnd() * 3.0f, rnd() * 3.0f};
        bad += check(sh, pos, cam, "random", k);
        ++cases;
    }
    const float special[3] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                              -std::numeric_limits<float>::infinity()};
    for (int f = 0; f < 48; ++f)
        for (float v : special) {
            for (float& c : sh) c = rnd();
            sh[f] = v;
            bad += check(sh, F3{rnd(), rnd(), rnd()}, cam, "special", f);
            ++cases;
        }
    for (float& c : sh) c = rnd();
    bad += check(sh, cam, cam, "at the camera", 0);
    ++cases;
    std::printf("%d cases, %d wrong\n", cases, bad);
    return bad != 0;
}
"""


def test_record_first_evaluation_against_the_coefficient_walk_on_the_host(tmp_path):
    from autovfx_amd import build
    cc = build.hipcc()
    src, exe = tmp_path / "sh_record_host.hip", tmp_path / "sh_record_host"
    src.write_text(PROGRAM)
    subprocess.check_call([cc, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-I", build.CSRC,
                           "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "2145 cases, 0 wrong" in out.stdout

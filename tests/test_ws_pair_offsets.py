"""The slim far N = 20 workspace layout (csrc/ntm_ws.h, WS::kPair): every vector the far
N = 20 kernels read by aligned pairs (ld_pair / ld5, csrc/ntm_lanes.h) starts on a 16-byte
offset, the reorder that put them there (uu to the head of the vector block) padded
nothing, and 16 workspaces still fit a CU's 160 KiB of LDS.  A second guard next to the
header's static_asserts: a host-only program prints the offsets the kernels use and the
test checks them.  No GPU."""
import os
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "mpc-ntm-control_amd" / "csrc"

PROGRAM = r"""
#include <cstdio>
#include "ntm_ws.h"
template <class W>
static void show(const char* tag) {
    std::printf("%s Phi %d\n%s e %d\n%s Gt %d\n%s Vb %d\n%s Uf %d\n%s xp %d\n%s irn %d\n%s U %d\n%s dr %d\n%s d %d\n",
                tag, W::oPhin(20), tag, W::oEn(20), tag, W::oGtn(20), tag, W::oVecn(20, 6), tag, W::oVecn(20, 7), tag,
                W::oXpn(20), tag, W::oIrnn(20), tag, W::oUn(20), tag, W::oDrn(20), tag, W::oVecn(20, 3));
    std::printf("%s a11 %d\n%s a21 %d\n%s vector_block %d\n%s F %d\n", tag, 3 * 20, tag, 4 * 20, tag, W::oVfar(20), tag,
                W::oVecn(20, 0));
    for (int l = 0; l < 20; ++l) std::printf("%s column %d\n", tag, W::oGtn(20) + W::gcoln(20, l));
}
int main() {
    show<ntm::WS<20, false, true>>("step");
    show<ntm::WS<20, true, true>>("gen");
    std::printf("ws_bytes %d\nws_doubles %d\n", ntm::ws_bytes(20, true), ntm::ws_doubles(20, true));
    return 0;
}
"""

PAIR_VECTORS = ("Phi", "e", "Gt", "Vb", "xp", "irn", "U", "dr", "d", "a11", "a21")


def test_pair_vectors_start_on_16_bytes(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "ws_offsets.hip"
    src.write_text(PROGRAM)
    exe = tmp_path / "ws_offsets"
    subprocess.run([hipcc, "-std=c++17", "--cuda-host-only", "-DNTM_N20_NO_RATE=1", f"-I{CSRC}", "-o", str(exe), str(src)],
                   check=True, timeout=300)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout
    print(out)
    vals = {}
    for ln in out.splitlines():
        *key, v = ln.split()
        vals.setdefault(" ".join(key), []).append(int(v))
    for tag in ("step", "gen"):
        for name in PAIR_VECTORS:
            (off,) = vals[f"{tag} {name}"]
            assert (8 * off) % 16 == 0, (tag, name, off)
        cols = vals[f"{tag} column"]
        assert len(cols) == 20 and all((8 * c) % 16 == 0 for c in cols), cols
        # uu (N + 1 doubles) leads the vector block, rinfo's 2N ints (N doubles) follow, then F .. Uf
        # (8 N-vectors) up to xp: Vb and Uf stay one 2N-vector, and nothing is padded
        (blk,), (f0,), (vb,), (uf,), (xp,) = (vals[f"{tag} {k}"] for k in ("vector_block", "F", "Vb", "Uf", "xp"))
        assert f0 == blk + 21 + 20 and vb == f0 + 6 * 20 and uf == vb + 20 and xp == uf + 20
    (nbytes,), (ndoubles,) = vals["ws_bytes"], vals["ws_doubles"]
    assert nbytes % 16 == 0 and 16 * nbytes <= 160 * 1024, nbytes
    assert nbytes == 10224 and ndoubles == 1197          # the layout's size before the reorder

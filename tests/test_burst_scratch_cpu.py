"""The scratch layouts of the burst entry points and of EPaxos (frankenpaxos_amd/csrc/fpx_scratch.hpp: the Carver, the four
layouts fpx_api.hip carves its buffers with and the three of fpx_epaxos.hip -- the multi-key prologue at n = 3, 5, 7, the
multi-key pair arrays, the leader-replies compaction) in a stand-alone program, tests/burst_scratch_main.cpp, built with
-fsanitize=address,undefined and run as its own program: for n in {0, 1, 255, 256, 257, 3000, 262 969} every array is
aligned for its type, inside the size the sizing pass returned, and disjoint from the others.  No GPU; nothing of the
library is loaded under a sanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_layout_is_aligned_disjoint_and_inside_its_size(tmp_path):
    exe = str(tmp_path / "burst_scratch")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o",
                            exe, os.path.join(ROOT, "tests", "burst_scratch_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "all layouts ok" and not [ln for ln in lines if ln.startswith("FAIL")]
    assert sum(ln.startswith("ok ") for ln in lines) == 7 * (5 + 5)          # seven sizes; four burst buffers (one in two
    # forms), the multi-key prologue at three replica counts, the pair arrays, the leader-replies compaction

"""The layout of a host-pointer call's arrays (frankenpaxos_amd/csrc/fpx_host_call.hpp: lay_stage, which host_call in
fpx_host.hpp consumes for both fpx_api.hip and fpx_epaxos.hip) in a stand-alone program, tests/host_call_layout_main.cpp,
built with -fsanitize=address,undefined and run as its own program.  Lists of arrays of 0, 1, 255, 256, 257 and 262 969
bytes, with an absent optional input first, in the middle and last, held arrays among plain ones (a held_first whose
length word comes after it), and the fill sequence NO_FILL, 0, 0, 0xFF, NO_FILL, 0: every offset is aligned, the arrays
are disjoint and in list order, the totals are the last ends, an absent input takes no space, the held offsets are 8-byte
aligned and disjoint, the fill runs cover exactly the filled arrays with neighbours of one value merged, and every span is
written into blocks of exactly the computed totals.  No GPU; nothing of the library is loaded under a sanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_list_is_aligned_disjoint_and_inside_its_totals(tmp_path):
    exe = str(tmp_path / "host_call_layout")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o",
                            exe, os.path.join(ROOT, "tests", "host_call_layout_main.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "all layouts ok" and not [ln for ln in lines if ln.startswith("FAIL")]
    # the empty list; six shifts of the sizes under the fill sequence; an absent input in three positions; six shifts of
    # the sizes over the list with held arrays
    assert sum(ln.startswith("ok ") for ln in lines) == 1 + 6 + 3 + 6

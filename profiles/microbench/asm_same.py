"""Do two builds of csrc/fpx_api.hip hold the same machine code, function by function?

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -Wno-unused-function --cuda-device-only -S -o before.s frankenpaxos_amd/csrc/fpx_api.hip
    ... edit ...
    hipcc (the same) -o after.s frankenpaxos_amd/csrc/fpx_api.hip
    python profiles/microbench/asm_same.py [--kernarg] before.s after.s [substring of the mangled names to look at]

Compares the instruction text of every function both files define (comments, directives and the numbering of local labels
dropped).  Used in round 5 to move the vote kernel's body into fpx_phase2_body.inc (a second kernel includes it) and the
division by multiplication into fpx_fastdiv.hpp WITHOUT touching what had been measured: all 130 k_phase2 instantiations
resp. all 186 device functions came out identical; wrapping the body in a __device__ function instead had changed every one
of the 130 (profiles/r05_cfg5.md).

--kernarg: a change that adds a member to a struct the kernels take by value (State::vote_sum, profiles/r09_vote_records.md)
moves every kernel argument behind it, and with it the offsets of the scalar loads and address sums that fetch them, in
kernels whose code is otherwise untouched.  With this switch the offset of EVERY s_load_dword* from a scalar register pair
and the hex literal of EVERY s_add_u32 are not compared, whichever pointer they belong to (the kernel-argument pointer is
copied between register pairs, so it cannot be told from the text of one instruction): "same" then means the same
instructions, registers and order up to such offsets, a weaker statement than without the switch."""
import re
import sys


KERNARG = False


def functions(path):
    out, name, buf = {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, buf = m.group(1), []
            out[name] = buf
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            name = None
            continue
        text = line.split(";")[0].rstrip()
        bare = text.strip()
        if not bare or (bare.startswith(".") and not bare.startswith(".LBB")):
            continue
        text = re.sub(r"\.LBB\d+_", ".LBB_", text)
        if KERNARG:
            text = re.sub(r"^(\s*s_load_dword\w*\s+[^,]+,\s*s\[\d+:\d+\],\s*)0x[0-9a-f]+", r"\1OFF", text)
            text = re.sub(r"^(\s*s_add_u32\s+s\d+,\s*s\d+,\s*)0x[0-9a-f]+$", r"\1OFF", text)
        buf.append(text)
    return out


def main():
    global KERNARG
    if "--kernarg" in sys.argv:
        KERNARG = True
        sys.argv.remove("--kernarg")
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    pattern = sys.argv[3] if len(sys.argv) > 3 else ""
    same, different = 0, []
    for name, body in a.items():
        if pattern not in name:
            continue
        if name not in b:
            print("only in", sys.argv[1], ":", name)
        elif body == b[name]:
            same += 1
        else:
            different.append((name, len(body), len(b[name])))
    for name in b:
        if pattern in name and name not in a:
            print("only in", sys.argv[2], ":", name)
    print("same", same, "different", len(different))
    for d in different[:50]:
        print("  %s: %d -> %d instructions" % d)
    return 1 if different else 0


if __name__ == "__main__":
    sys.exit(main())

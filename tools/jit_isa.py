"""Disassembles the run-time compiled kernel of a block system (no device needed): the code object hiprtc makes for
`gen_big_problem.py N [true]`, through the on-disk cache, as text + a one-line summary per entry (registers, spills, scratch)
and, per entry, a static count of the instructions of its system loop.  Used to check that an edit of jit_kernel.hip.hpp left
a kernel it should not touch instruction for instruction the same, and to steer one that it should:
python tools/jit_isa.py 500 /tmp/before.s ; <edit> ; python tools/jit_isa.py 500 /tmp/after.s

The system loop of an entry is taken to be the backward branch with the longest span; everything between its target and the
branch is counted once, whether a pass executes it or not (cold blocks the compiler laid out inside the span included), so the
figures compare builds of the same kernel and are an upper bound of what a wavefront issues per system."""
import glob
import os
import re
import struct
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def loop_counts(text):
    """{entry: {what: count}} over each entry's longest backward branch (objdump text with its `// address:` comments)."""
    out = {}
    for name, body in re.findall(r"^[0-9a-f]+ <(\w+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", text, re.M | re.S):
        ins = [(int(a, 16), op, arg.strip()) for op, arg, a in re.findall(r"^\s*([a-z_0-9]+)(.*?)//\s*([0-9A-F]+):", body, re.M)]
        span = None
        for addr, op, arg in ins:
            if op.startswith(("s_cbranch", "s_branch")) and re.match(r"\d+$", arg.split()[0]):
                off = int(arg.split()[0])
                target = addr + 4 + 4 * (off - 65536 if off >= 32768 else off)
                if target <= addr and (span is None or addr - target > span[1] - span[0]):
                    span = (target, addr)
        if span is None:
            continue
        ops = [op for addr, op, _ in ins if span[0] <= addr <= span[1]]
        n = lambda pred: sum(1 for op in ops if pred(op))
        out[name] = {
            "all": len(ops),
            "valu": n(lambda op: op.startswith("v_")),
            "salu": n(lambda op: op.startswith("s_") and op not in ("s_waitcnt", "s_nop", "s_barrier", "s_endpgm")),
            "f64_arith": n(lambda op: re.match(r"v_(add|mul|fma)_f64", op) is not None),
            "v_readlane": n(lambda op: op.startswith("v_readlane")),
            "v_writelane": n(lambda op: op.startswith("v_writelane")),
            "v_cndmask": n(lambda op: op.startswith("v_cndmask")),
            "v_cmp": n(lambda op: op.startswith("v_cmp")),
            "v_max_f64": n(lambda op: op.startswith("v_max_f64")),
            "v_mov": n(lambda op: op.startswith("v_mov")),
            "scratch": n(lambda op: op.startswith("scratch_")),
            "lds": n(lambda op: op.startswith("ds_")),
            "vmem": n(lambda op: op.startswith(("buffer_", "global_", "flat_"))),
        }
    return out


def main():
    n = int(sys.argv[1])
    out = sys.argv[2]
    over = len(sys.argv) > 3 and sys.argv[3] == "true"
    d = tempfile.mkdtemp(prefix="ezpz_isa_")
    os.environ["EZPZ_JIT_CACHE_DIR"] = d
    import ezpz_amd as E

    p = E.textual.Problem.from_str(E.textual.gen_big_problem(n, over)).to_constraint_system()
    src = E.specialized_source(p.records, p.num_vars, compile="cached")
    assert src
    (path,) = glob.glob(d + "/*.co")
    blob = open(path, "rb").read()
    magic, tag_b, src_b, code_b, _ = struct.unpack("<8sQQQQ", blob[:40])
    code = blob[40 + tag_b + src_b:40 + tag_b + src_b + code_b]
    co = os.path.join(d, "k.co")
    open(co, "wb").write(code)
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    # hiprtc hands out a fat binary or a plain code object; unbundle if needed
    if code[:4] != b"\x7fELF":
        subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang-offload-bundler", "--type=o", "--unbundle", "--input=" + co,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co + ".elf"])
        co = co + ".elf"
    text = subprocess.check_output([objdump, "-d", "--no-show-raw-insn", co]).decode()
    loops = loop_counts(text)
    text = re.sub(r"^\s*([a-z_0-9]+ .*?)\s*//\s*[0-9A-F]+:.*$", r"\1", text, flags=re.M)
    open(out, "w").write(text)
    notes = subprocess.check_output(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", co]).decode()
    for m in re.finditer(r"\.name:\s+(\S+).*?\.sgpr_count:\s+(\d+).*?\.sgpr_spill_count:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", notes, re.S):
        print("%s: sgpr %s (spilled %s) vgpr %s (spilled %s)" % m.groups(), end="")
        scratch = re.search(r"\.name:\s+%s\b.*?\.private_segment_fixed_size:\s+(\d+)" % re.escape(m.group(1)), notes, re.S)
        print(" scratch %s B" % (scratch.group(1) if scratch else "?"))
        if m.group(1) in loops:
            print("    loop: " + " ".join("%s %d" % kv for kv in loops[m.group(1)].items()))
    print("instructions:", len(re.findall(r"^\s*([sv]|global|ds|buffer|flat|scratch)_", text, re.M)))


main()

#!/usr/bin/env python3
"""Compare the device code of the library between two trees, kernel by kernel.

    tools/compare_kernels.py PARENT THIS                      two trees; an argument that is no directory is a commit of this
                                                              repository and is extracted with `git archive`
    tools/compare_kernels.py a.s a.log b.s b.log              two pairs of files: the assembly and the compiler's remarks

A tree is compiled with

    hipcc --offload-arch=gfx950 --offload-device-only -O3 -std=c++17 -ffp-contract=off -Rpass-analysis=kernel-resource-usage -S

(needs no GPU).  The assembly is split by kernel symbol, block labels are normalised and comments dropped; the remarks give each
kernel's registers, scratch, occupancy, spills and LDS.  Prints the summary in the format of profiles/*/resource_usage.txt:
kernels on each side, missing, new, resource usage differing, instructions differing, with the names.  Exit status 1 if anything
is missing or differs.  The tool compares text; it looks for nothing inside the code.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

FLAGS = ["--offload-arch=gfx950", "--offload-device-only", "-O3", "-std=c++17", "-ffp-contract=off",
         "-Rpass-analysis=kernel-resource-usage", "-S"]
SOURCE = os.path.join("torchpdlp_amd", "csrc", "pdlp_hip.hip")
FIELDS = ["TotalSGPRs", "VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]"]
HEADER = "  SGPR   VGPR   scr   occ   sSp   vSp   LDS  kernel"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compile_tree(tree, out_dir, tag):
    """-> (assembly path, remark log path) of `tree`; a commit is extracted first"""
    if not os.path.isdir(tree):
        src = os.path.join(out_dir, tag + "_tree")
        os.makedirs(src)
        archive = subprocess.run(["git", "-C", REPO, "archive", tree, "torchpdlp_amd/csrc", "include"], check=True, capture_output=True)
        subprocess.run(["tar", "-x", "-C", src], input=archive.stdout, check=True)
        tree = src
    asm, log = os.path.join(out_dir, tag + ".s"), os.path.join(out_dir, tag + ".log")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    with open(log, "w") as f:
        # (relative paths: the remarks of both trees then name the same files)
        subprocess.run([hipcc] + FLAGS + ["-I", "include", SOURCE, "-o", os.path.abspath(asm)], cwd=tree, stderr=f, check=True)
    return asm, log


def split_kernels(asm_path):
    """-> {symbol: [normalised instruction lines]} for every kernel (a function with an .amdhsa_kernel block)"""
    start = re.compile(r"^([A-Za-z_][\w$.]*):\s*; @\1\s*$")
    label = re.compile(r"\.L([A-Za-z]+)\d+_")
    bodies, kernels, name = {}, set(), None
    with open(asm_path) as f:
        for line in f:
            m = start.match(line)
            if m:
                name = m.group(1)
                bodies[name] = []
                continue
            if line.startswith("\t.amdhsa_kernel "):
                kernels.add(line.split()[1])
            if name is None:
                continue
            if line.startswith(".Lfunc_end") or line.startswith("\t.section"):
                name = None
                continue
            text = label.sub(r".L\1_", line.split(";")[0].rstrip())
            if text.strip():
                bodies[name].append(text)
    return {k: v for k, v in bodies.items() if k in kernels}


def resource_usage(log_path):
    """-> {symbol: tuple of the seven figures} from the kernel-resource-usage remarks"""
    usage, name = {}, None
    pat = re.compile(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis=kernel-resource-usage\]")
    with open(log_path) as f:
        for line in f:
            m = pat.search(line)
            if not m:
                continue
            key, val = m.group(1).strip(), m.group(2)
            if key == "Function Name":
                name = val
                usage[name] = {}
            elif name is not None and key in FIELDS:
                usage[name][key] = int(val)
    return {k: tuple(v.get(f, -1) for f in FIELDS) for k, v in usage.items()}


def demangle(symbols):
    """-> {symbol: readable name}: demangled, without the anonymous namespace, the return type and the argument list"""
    symbols = sorted(symbols)
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    for cand in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"):
        if tool is None and os.path.exists(cand):
            tool = cand
    if tool is None or not symbols:
        return {s: s for s in symbols}
    out = subprocess.run([tool], input="\n".join(symbols) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    names = {}
    for sym, d in zip(symbols, out):
        d = d.replace("(anonymous namespace)::", "")
        if d.endswith(")"):                       # cut the argument list: the parenthesis that matches the last one
            depth = 0
            for i in range(len(d) - 1, -1, -1):
                depth += (d[i] == ")") - (d[i] == "(")
                if depth == 0:
                    d = d[:i]
                    break
        names[sym] = d[5:] if d.startswith("void ") else d
    return names


def row(u, name):
    return "  %6d %6d %6d %6d %6d %6d %6d  %s" % (u + (name,))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("paths", nargs="+", help="PARENT THIS (trees or commits), or a.s a.log b.s b.log")
    ap.add_argument("--keep", metavar="DIR", help="compile into DIR and keep the assembly and the remarks there")
    args = ap.parse_args()
    tmp = None
    if len(args.paths) == 2:
        out_dir = args.keep or (tmp := tempfile.mkdtemp(prefix="compare_kernels_"))
        os.makedirs(out_dir, exist_ok=True)
        (asm_a, log_a), (asm_b, log_b) = compile_tree(args.paths[0], out_dir, "parent"), compile_tree(args.paths[1], out_dir, "this")
    elif len(args.paths) == 4:
        asm_a, log_a, asm_b, log_b = args.paths
    else:
        ap.error("two trees or four files")
    ka, kb = split_kernels(asm_a), split_kernels(asm_b)
    ua, ub = resource_usage(log_a), resource_usage(log_b)
    if tmp:
        shutil.rmtree(tmp)
    names = demangle(set(ka) | set(kb))
    common = sorted(set(ka) & set(kb), key=names.get)
    missing = sorted(set(ka) - set(kb), key=names.get)
    new = sorted(set(kb) - set(ka), key=names.get)
    res_diff = [k for k in common if ua.get(k) != ub.get(k)]
    no_remark = [k for k in common if k not in ua or k not in ub]       # (a log that was not parsed must not read as "0 differ")
    ins_diff = [k for k in common if ka[k] != kb[k]]

    print("hipcc " + " ".join(FLAGS))
    print("Columns: total SGPRs, VGPRs, scratch bytes per lane, occupancy in waves per SIMD, spilled SGPRs, spilled VGPRs, LDS bytes per block.")
    print()
    print("kernels in the parent: %d; in this commit: %d; missing here: %d; new: %d" % (len(ka), len(kb), len(missing), len(new)))
    print("kernels of the parent whose resource usage differs here: %d" % len(res_diff))
    if no_remark:
        print("kernels without a resource-usage remark on one side or both: %d" % len(no_remark))
    print("kernels of the parent whose instructions differ here (device assembly, block labels normalised): %d of %d compared"
          % (len(ins_diff), len(common)))
    for title, syms, table in (("Missing kernels", missing, ua), ("New kernels", new, ub)):
        if syms:
            print("\n%s\n%s" % (title, HEADER))
            for k in syms:
                print(row(table.get(k, (-1,) * 7), names[k]))
    if res_diff:
        print("\nResource usage differs (parent, then this commit)\n" + HEADER)
        for k in res_diff:
            print(row(ua.get(k, (-1,) * 7), names[k]))
            print(row(ub.get(k, (-1,) * 7), ""))
    if ins_diff:
        print("\nInstructions differ (lines in the parent / here)")
        for k in ins_diff:
            print("  %6d %6d  %s" % (len(ka[k]), len(kb[k]), names[k]))
    return 1 if (missing or res_diff or ins_diff or no_remark) else 0


if __name__ == "__main__":
    sys.exit(main())

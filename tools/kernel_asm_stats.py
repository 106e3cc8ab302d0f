"""Load / wait counts of the kernels in a gfx950 assembly listing, next to the compiler's resource remarks.

  hipcc <flags of build.py> -x hip --cuda-device-only -S csrc/FILE.hip -o FILE.s -Rpass-analysis=kernel-resource-usage 2> FILE.rpass
  python tools/kernel_asm_stats.py FILE.s FILE.rpass [substring of the demangled kernel name ...]

Per kernel: VGPRs / AGPRs / scratch bytes (the remarks), scalar wait rounds (s_waitcnt with lgkmcnt) in front of the first
vector memory load, vector memory loads, s_waitcnt instructions that name vmcnt and how many of them are vmcnt(0), scalar
waits and branches in all.  Static counts of the listing: what a wave executes depends on the path it takes."""
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
        return dict(zip(names, out))
    except OSError:
        return {n: n for n in names}


def remarks(path):
    """{mangled name: {field: value}} from -Rpass-analysis=kernel-resource-usage"""
    res, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: .*?\s{2,}(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|SGPRs|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    return res


def kernels(path):
    """{mangled name: [instruction lines]} of the .s file"""
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            t = line.strip()
            if t and not t.startswith((";", ".")):
                cur.append(t)
    return out


def stats(ins):
    is_vload = lambda t: re.match(r"(buffer_load|global_load|flat_load|scratch_load)", t) is not None
    first = next((i for i, t in enumerate(ins) if is_vload(t)), len(ins))
    lgkm = lambda t: t.startswith("s_waitcnt") and "lgkmcnt" in t
    vm = [t for t in ins if t.startswith("s_waitcnt") and "vmcnt" in t]
    return dict(scalar_waits_before_first_vload=sum(1 for t in ins[:first] if lgkm(t)), vloads=sum(1 for t in ins if is_vload(t)),
                vmcnt_waits=len(vm), vmcnt0=sum(1 for t in vm if re.search(r"vmcnt\(0\)", t)),
                lgkm_waits=sum(1 for t in ins if lgkm(t)), branches=sum(1 for t in ins if t.startswith(("s_cbranch", "s_branch"))))


def main():
    s_path, r_path, want = sys.argv[1], sys.argv[2], sys.argv[3:]
    ks, rm = kernels(s_path), remarks(r_path)
    names = demangle(list(ks))
    for mangled, ins in ks.items():
        name = names[mangled]
        if want and not any(w in name for w in want):
            continue
        st, r = stats(ins), rm.get(mangled, {})
        print("%s\n    VGPR %s AGPR %s scratch %s | scalar waits before first vector load %d | vector loads %d, vmcnt waits %d (vmcnt(0): %d) | "
              "lgkmcnt waits %d, branches %d" % (re.sub(r"^void \(anonymous namespace\)::", "", name), r.get("VGPRs", "?"), r.get("AGPRs", "?"),
                                                  r.get("ScratchSize", "?"), st["scalar_waits_before_first_vload"], st["vloads"], st["vmcnt_waits"],
                                                  st["vmcnt0"], st["lgkm_waits"], st["branches"]))


if __name__ == "__main__":
    main()

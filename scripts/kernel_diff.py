"""Compare the kernels of one translation unit between two builds, without a GPU (dev tool):
    python scripts/kernel_diff.py OLD_DIR NEW_DIR [UNIT]
Each directory holds what
    hipcc <the flags of sapr_amd/build.py> -save-temps=obj -Rpass-analysis=kernel-resource-usage \\
          -c sapr_amd/csrc/UNIT.hip -o DIR/UNIT.o 2> DIR/log.txt
leaves behind (run it inside DIR, once per source tree): the gfx950 assembly and the resource remarks.  Prints one line
per kernel of NEW_DIR: registers, spills, scratch, occupancy, LDS, and — for a kernel OLD_DIR has too — whether its
resource figures and its instruction text are the same (comments, debug directives and the numbering of local labels,
which counts the functions in front, set aside), with a hash of the text.  UNIT defaults to connected_embed."""
import hashlib
import re
import subprocess
import sys


def resources(log):
    out, cur = {}, None
    for line in open(log):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        m = re.search(r"remark: .*?:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", line)
        if m and cur:
            out[cur][m.group(1).strip()] = int(m.group(2))
    return out


def bodies(asm):
    """Mangled name -> the instruction text between the function's label and its end."""
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", open(asm).read(), flags=re.S | re.M):
        lines = [re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r";.*", "", ln)).rstrip() for ln in m.group(2).splitlines()]
        out[m.group(1)] = "\n".join(ln for ln in lines if ln and not ln.strip().startswith((".loc", ".file", ".cfi")))
    return out


def main():
    old, new = sys.argv[1], sys.argv[2]
    unit = sys.argv[3] if len(sys.argv) > 3 else "connected_embed"
    asm = f"{unit}-hip-amdgcn-amd-amdhsa-gfx950.s"
    r_old, r_new = resources(f"{old}/log.txt"), resources(f"{new}/log.txt")
    b_old, b_new = bodies(f"{old}/{asm}"), bodies(f"{new}/{asm}")
    names = sorted(r_new)
    plain = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines()
    changed = 0
    for name, full in zip(names, plain):
        r = r_new[name]
        short = re.sub(r"\(anonymous namespace\)::|^void |sapr::", "", full).split("(")[0]
        line = (f"{short:34s} VGPR {r.get('VGPRs'):3d} AGPR {r.get('AGPRs'):2d} spills s{r.get('SGPRs Spill')}/"
                f"v{r.get('VGPRs Spill')} scratch {r.get('ScratchSize')} occupancy {r.get('Occupancy')} "
                f"LDS {r.get('LDS Size')}")
        if name in r_old:
            same_r, same_t = r_old[name] == r, b_old.get(name) == b_new.get(name)
            changed += not (same_r and same_t)
            line += (f" | resources {'same' if same_r else 'DIFFER'}, text {'same' if same_t else 'DIFFER'} "
                     f"{hashlib.sha256(b_new[name].encode()).hexdigest()[:12]}")
        else:
            line += " | new"
        print(line)
    gone = sorted(set(r_old) - set(r_new))
    print(f"{len(names)} kernels, {len(set(names) & set(r_old))} in both builds, {changed} changed, {len(gone)} gone")
    return 1 if changed or gone else 0


if __name__ == "__main__":
    sys.exit(main())

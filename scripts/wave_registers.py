"""Registers of the wave-private MFCC kernels, from a device-only compile of mfcc.hip with the build's own flags
(no GPU needed):
    python scripts/wave_registers.py [--all]
Prints VGPRs (and what the 8-register granule makes of them), scratch and spills of every mfcc_wave_kernel and
mfcc_wave_finish_kernel instantiation (--all: of every kernel of the unit) as the compiler reports them
(-Rpass-analysis=kernel-resource-usage), and the register budget of a SIMD lane for the headline pair: four spectral
wavefronts of <false, 1, 15, 7> and one finish wavefront of <10, false> (scripts/experiments/README.md, "resident finish
pass")."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sapr_amd import build as B  # noqa: E402

GRANULE = 8
def readable(mangled):
    """mfcc_wave_kernel<false, 1, 15, 7> from the Itanium name (the template arguments are bools and ints)."""
    m = re.search(r"\d+(mfcc_wave_kernel|mfcc_wave_finish_kernel)I((?:L[bi]\d+E)+)", mangled)
    if not m:
        m = re.search(r"_GLOBAL__N_1\d+([A-Za-z_0-9]+?)(?:I|E)", mangled)
        return m.group(1) if m else mangled
    args = [("true" if v == "1" else "false") if t == "b" else v for t, v in re.findall(r"L([bi])(\d+)E", m.group(2))]
    return f"{m.group(1)}<{', '.join(args)}>"


def main():
    with tempfile.TemporaryDirectory(prefix="sapr_regs_") as tmp:
        cmd = [B._hipcc(), *B.FLAGS, *B._extra_flags(), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
               "-c", os.path.join(B.CSRC, "mfcc.hip"), "-o", os.path.join(tmp, "mfcc.o")]
        txt = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows = []
    for blk in re.split(r"remark: [^\n]*Function Name: ", txt)[1:]:
        def field(key):
            m = re.search(re.escape(key) + r": (\d+)", blk)
            return int(m.group(1)) if m else -1
        rows.append((blk.split()[0], field("VGPRs"), field("ScratchSize [bytes/lane]"), field("VGPRs Spill"),
                     field("Occupancy [waves/SIMD]")))
    names = [readable(r[0]) for r in rows]
    show_all, alloc = "--all" in sys.argv, {}
    print(f"{'kernel':44s} {'VGPRs':>5s} {'alloc':>5s} {'scratch':>7s} {'spills':>6s} {'waves/SIMD':>10s}")
    for name, (_, vgprs, scratch, spills, occ) in zip(names, rows):
        if not show_all and not name.startswith(("mfcc_wave_kernel", "mfcc_wave_finish_kernel")):
            continue
        alloc[name] = (vgprs + GRANULE - 1) // GRANULE * GRANULE
        print(f"{name:44s} {vgprs:5d} {alloc[name]:5d} {scratch:7d} {spills:6d} {occ:10d}")
    spec, fin = alloc["mfcc_wave_kernel<false, 1, 15, 7>"], alloc["mfcc_wave_finish_kernel<10, false>"]
    print(f"4 x spectral <false, 1, 15, 7> + 1 x finish <10, false> = 4 x {spec} + {fin} = {4 * spec + fin} of 512 registers "
          f"per SIMD lane: the finish wavefront is {'' if 4 * spec + fin <= 512 else 'NOT '}resident beside a full spectral grid")
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Are the kernels two builds share the same instructions?  Compares, symbol by symbol, the gfx950 device assembly hipcc leaves with
--save-temps (<unit>-hip-amdgcn-amd-amdhsa-gfx950.s) in two directories: comments are stripped, the per-function index of local labels
(.LBB<n>_) and the per-file __hip_cuid_<hash> symbol are normalised (a kernel added in front shifts the first, the second hashes the
source path).  Symbols only one side has are listed, not compared.  No GPU needed.

  for u in $(sed -n 's/^SRCS *:= *//p' rmcv_amd/csrc/Makefile | sed 's/\.hip//g'); do        (every unit of the Makefile's SRCS)
    (cd DIR && hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math --save-temps -c ROOT/rmcv_amd/csrc/$u.hip -o $u.o); done
  python tools/isa_identity.py BEFORE_DIR AFTER_DIR [unit ...]        exit status 1 if a shared symbol differs

A kernel that has moved to another unit (k_image_export: rmcv_host -> rmcv_frame) is compared by concatenating the two units' .s files
of the side that split them under the name of the unit that held it before."""
import glob
import os
import re
import sys

SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"


def symbols(path):
    out, cur = {}, None
    for ln in open(path):
        m = re.match(r"^(_Z\w+):\s", ln)
        if m and cur is None:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        if ln.startswith(".Lfunc_end"):
            cur = None
            continue
        ln = re.sub(r";.*", "", ln).rstrip()
        ln = re.sub(r"(\.L[A-Za-z_]*?)\d+_", r"\1N_", ln)
        out[cur].append(re.sub(r"__hip_cuid_\w+", "__hip_cuid", ln))
    return out


before, after = sys.argv[1], sys.argv[2]
units = sys.argv[3:] or sorted(os.path.basename(p)[:-len(SUFFIX)] for p in glob.glob(os.path.join(before, "*" + SUFFIX)))
bad = 0
for u in units:
    a, b = symbols(os.path.join(before, u + SUFFIX)), symbols(os.path.join(after, u + SUFFIX))
    shared = [k for k in a if k in b]
    diff = [k for k in shared if a[k] != b[k]]
    bad += len(diff)
    print("%-16s %2d shared symbols, %d differ; only before: %d, only after: %d" % (u, len(shared), len(diff), len(a) - len(shared), len(b) - len(shared)))
    for k in diff:
        print("   DIFFERS  " + k)
sys.exit(1 if bad else 0)

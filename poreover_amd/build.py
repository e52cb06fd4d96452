"""Build libporeover_hip.so in-tree with hipcc for gfx950 (MI355X).  No JIT cache, no torch
extension machinery: the .so sits next to the sources so it travels with the repo snapshot."""
import os
import shlex
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libporeover_hip.so")
SOURCES = ["po_capi.hip", "po_ctc.hip", "po_falign.hip", "po_viterbi.hip", "po_beam1d.hip", "po_beam2d.hip", "po_beam2d_grid.hip", "po_beam2d_route.hip", "po_beam2d_reg.hip", "po_pair.hip", "po_lattice.hip", "po_prefix.hip", "po_ingest.hip", "po_ingest_strided.hip", "po_gamma.hip", "po_stream.hip", "po_call.hip", "po_train.hip", "po_train_group.hip", "po_map.hip", "po_label.hip", "po_qual.hip", "po_basecall.hip", "po_fastq.hip", "po_pair_basecall.hip", "po_eval.hip", "po_acc.hip", "po_aln.hip", "po_prep.hip", "po_basecall_stream.hip", "po_skip.hip", "po_pair_basecall_stream.hip"]
HEADERS = ["po_device.h", os.path.join("..", "..", "include", "poreover_hip.h")]
# The pair beam search is four sources: po_beam2d.hip (beam2d_kernel), po_beam2d_grid.hip (beam2d_grid_kernel), po_beam2d_reg.hip
# (beam2d_reg_kernel) and po_beam2d_route.hip (the host layer that chooses among them, with the pre-pass and walk kernels).
# Per-object compiler options (measured, round 6: profiles/r06_ab_compiler_flags.txt).  -amdgpu-use-amdgpu-trackers (the AMDGPU register-pressure
# trackers in the machine scheduler) is worth 1 % on the 32-slot pair kernel, costs 1.5 % on the 64-slot pair kernel and 5 % on beam2d_kernel's
# W = 25 class; in po_beam1d.hip it gives beam1d_wave_kernel 1.5 % and takes 4.5 % from beam1d_kernel (W = 25), so that file goes without.
# po_beam2d_reg.hip is compiled twice (PO_REG_TU: the 32-slot kernels + the C entry points | the 64-slot kernels), each object with what it
# runs best with.  (object name, source, extra options)
TRACKERS = ["-mllvm", "-amdgpu-use-amdgpu-trackers"]
OBJECTS = [(s, s, []) for s in SOURCES if s != "po_beam2d_reg.hip"] + [
    ("po_beam2d_reg.hip", "po_beam2d_reg.hip", ["-DPO_REG_TU=1"] + TRACKERS),
    ("po_beam2d_reg_wide.hip", "po_beam2d_reg.hip", ["-DPO_REG_TU=2"]),
]


FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unused-value", "-Wno-unused-function"]


def compile_cmd(oname, extra=()):
    """The command that compiles object `oname` of OBJECTS, without its -c / -o tail: what build() runs, and what the variant and ISA
    scripts ask for (--cmd), so that they compile what the product compiles.  A bare name gets .hip.  po_beam2d_reg.hip names the
    library's first object of that source (PO_REG_TU=1, the 32-slot kernels); append -UPO_REG_TU for the whole file with that
    object's options, as scripts/build_file_variant.sh does."""
    if not oname.endswith(".hip"):
        oname += ".hip"
    sname, opts = next(((s, x) for o, s, x in OBJECTS if o == oname), (oname, []))
    return [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *FLAGS, *opts, *extra, os.path.join(CSRC, sname)]


def _newest(paths):
    return max(os.path.getmtime(p) for p in paths)


def build(force=False, verbose=False):
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    deps = srcs + [os.path.normpath(os.path.join(CSRC, h)) for h in HEADERS]
    deps += [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not force and os.path.exists(LIB) and os.path.getmtime(LIB) >= _newest(deps + [os.path.abspath(__file__)]):
        return LIB
    objs = []
    os.makedirs(os.path.join(CSRC, "_obj"), exist_ok=True)
    me = os.path.abspath(__file__)   # (the options live here)
    for oname, sname, _ in OBJECTS:
        s = os.path.join(CSRC, sname)
        o = os.path.join(CSRC, "_obj", oname + ".o")
        if force or not os.path.exists(o) or os.path.getmtime(o) < _newest([s, me] + deps[len(srcs):]):
            cmd = compile_cmd(oname) + ["-c", "-o", o]
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            subprocess.check_call(cmd)
        objs.append(o)
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", LIB]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    if "--cmd" in sys.argv:   # build.py --cmd OBJECT [extra flags]
        i = sys.argv.index("--cmd")
        print(shlex.join(compile_cmd(sys.argv[i + 1], sys.argv[i + 2:])))   # (quoted for the shell: eval it)
    else:
        print(build(force="--force" in sys.argv, verbose=True))

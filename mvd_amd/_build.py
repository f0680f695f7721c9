"""Build libmvd_hip.so (gfx950) in-tree with hipcc.  No JIT cache: the .so travels with the repo snapshot."""
import glob
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libmvd_hip.so")
SOURCES = ["gemm.hip", "gemm_relu.hip", "gemm_pp.hip", "gemm_sm.hip", "gemm_xs.hip", "conv_ws.hip", "attention.hip", "norm.hip", "misc.hip", "freeu.hip", "tome.hip", "todo.hip", "sched.hip", "apg.hip", "unipc.hip", "losses.hip", "engine.hip", "vae.hip", "text.hip", "vision.hip", "vgg.hip", "lpips.hip", "fid.hip", "kid.hip", "prdc.hip", "imageio.hip"]
# measurement-only experiment kernels: linked by tools/build_variant.py into probe builds (-DMVD_PROBE), never into the product
PROBE_SOURCES = ["probe/gemm_ring.hip"]     # (+ probe/attention_probe*.inc, included by attention.hip under -DMVD_PROBE)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# -packed-fp32-ops (device code generation without v_pk_{fma,mul,add}_f32): a PRECAUTION against an unexplained fault.  The
# four-pixel conv_out probe kernel (csrc/probe/conv_out4.inc, not shipped) gave run-to-run differences when two processes shared
# one GPU; the differences went away with scalar v_fma_f32 and when exactly its 38 `v_pk_fma_f32 ... op_sel:[0,1,0]` were
# rewritten in the assembly (profiles/r04_probe_conv_out4_diagnosis.log).  That localises the fault to an
# instruction form; the root cause is NOT known (a wave context save/restore or time-slicing problem that the changed register
# allocation merely hides fits the same evidence).  The product is built without that instruction class: same IEEE operation per
# element (outputs bit-identical), 0-0.3 % of a step.  The flag reaches both passes: hipcc 7.2 refuses to forward -Xclang through
# -Xarch_device and silently ignores `-Xarch_device -mno-packed-fp32-ops` (checked: the packed instruction is still selected), so
# the host pass's "'-packed-fp32-ops' is not a recognized feature" note is dropped from the build output below instead.
NO_PACKED_FP32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
HOST_PASS_NOISE = "'-packed-fp32-ops' is not a recognized feature for this target"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", *NO_PACKED_FP32]


def _stale(out, deps):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    hdrs = sorted(glob.glob(os.path.join(CSRC, "*.h"))) + [os.path.join(HERE, "..", "include", "mvd_hip.h")]
    objdir = os.path.join(CSRC, "build")
    os.makedirs(objdir, exist_ok=True)
    jobs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace(".hip", ".o"))
        if force or _stale(o, [s] + hdrs):
            jobs.append([HIPCC, *FLAGS, "-c", s, "-o", o])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed: {' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
        return "\n".join(ln for ln in r.stderr.splitlines() if HOST_PASS_NOISE not in ln)

    with ThreadPoolExecutor(max_workers=4) as ex:
        for warn in ex.map(run, jobs):
            if warn and verbose:
                print(warn, file=sys.stderr)
    objs = [os.path.join(objdir, s.replace(".hip", ".o")) for s in SOURCES]
    if force or jobs or _stale(LIB, objs):
        run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB, *objs])
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))

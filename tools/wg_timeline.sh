#!/bin/bash
# Profiling build of the library with per-workgroup timestamps in the striped and the queued
# lookup (-DET_WG_TIMELINE): tools/tl/libembtab_hip.so.  The package's own library is untouched.
# Only et_lookup.hip is compiled again; the other objects are the package build's, taken from
# the build's own unit list (__graft_entry__.UNITS), so the link never goes stale.
# EXTRA_DEFINES="ET_EXPERIMENTS" adds the knobs (ET_AFFINITY ...); TL_NAME=x writes
# tools/tl/libembtab_hip_x.so instead.
# Build here (CPU), run tools/wg_timeline.py on the GPU box (ET_TL_LIBRARY picks the library).
set -e
cd "$(dirname "$0")/.."
mkdir -p tools/tl
SUF=$([ -z "$TL_NAME" ] && echo "" || echo "_$TL_NAME")
python3 - <<PY
import os, subprocess
import __graft_entry__ as g
g.build_hip()
hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
defs = ["ET_WG_TIMELINE"] + "${EXTRA_DEFINES:-}".split()
obj = "tools/tl/et_lookup_tl$SUF.o"
subprocess.run([hipcc, *g.HIPCC_FLAGS, *(f"-D{d}" for d in defs), f"-I{g.INCLUDE}", "-c",
                os.path.join(g.CSRC, "et_lookup.hip"), "-o", obj], check=True)
objs = [obj if u == "et_lookup.hip" else os.path.join(g.OBJ_DIR, os.path.splitext(u)[0] + ".o")
        for u in g.UNITS]
subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o",
                "tools/tl/libembtab_hip$SUF.so", *objs, *g.LINK_LIBS], check=True)
os.remove(obj)
PY
echo built tools/tl/libembtab_hip$SUF.so

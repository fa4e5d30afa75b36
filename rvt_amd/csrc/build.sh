#!/bin/bash
# Build librvt_hip.so (gfx950 code objects + host launchers) in-tree: `make -j` over the capi_*.hip parts (PARTS of the Makefile),
# on at most 16 jobs: nproc reports the whole host, also where a job may use only a share of it.
# A failed compile fails the script (pipefail: the grep only drops empty lines) — a stale library never passes for a fresh one.
set -e -o pipefail
cd "$(dirname "$0")"
jobs=$(nproc)
make -j"$((jobs < 16 ? jobs : 16))" "$@" 2>&1 | { grep -v "^$" || true; }
test -f ../librvt_hip.so
test ! ../librvt_hip.so -ot _obj/capi_core.o
echo "built $(realpath ../librvt_hip.so)"

#!/bin/bash
# Build libmfm_hip.so for gfx950 in-tree (cross-compiles without a GPU); incremental through the Makefile.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
# at most 16 compile jobs: on a shared host nproc can count CPUs this job may not use
JOBS=$(nproc)
[ "$JOBS" -gt 16 ] && JOBS=16
make -C "$HERE" -f "$HERE/Makefile" -j"$JOBS" "$@"

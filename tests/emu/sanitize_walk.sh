#!/bin/bash
# TEST-ONLY: segment walks of sanitize_walk.cpp (the scan's walk kinds, mt_walk_segments) on the
# engine's host emulation, one executable under AddressSanitizer + UndefinedBehaviorSanitizer
# (host code only; no GPU).
# usage: tests/emu/sanitize_walk.sh [outdir]   (exit status != 0 on any report or mismatch)
set -e
HERE=$(cd "$(dirname "$0")" && pwd)
OUT=${1:-/tmp/mt_sanitize}
mkdir -p "$OUT"
g++ -O1 -g -std=c++17 -pthread -Wno-unknown-pragmas -DMT_G_MWMIN=64 -DMT_BPC_CHECK=1 \
    -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer \
    -o "$OUT/sanitize_walk" "$HERE/sanitize_walk.cpp"
ASAN_OPTIONS=halt_on_error=1:detect_stack_use_after_return=1 \
UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 "$OUT/sanitize_walk"

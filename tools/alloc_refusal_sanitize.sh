#!/bin/bash
# tools/alloc_refusal_sanitize.sh — AddressSanitizer + UBSan run, leak detection on, of the stand-alone sweep of refused allocations over the shared
# drivers (tools/alloc_refusal_check.cpp: its own main, no Python, no GPU).  Exit status 0 and "failures": 0 when clean.
set -e
cd "$(dirname "$0")/.."
mkdir -p tests/_build
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wno-unknown-pragmas -I stark_mlwe_amd/csrc \
    tools/alloc_refusal_check.cpp -o tests/_build/alloc_refusal_check
ASAN_OPTIONS=detect_leaks=1 ./tests/_build/alloc_refusal_check

#!/bin/bash
# tools/ntt_plan_sanitize.sh — AddressSanitizer + UBSan run of the stand-alone host check of the batched NTT / LDE launch plan and its one-shape
# predicate (tools/ntt_plan_check.cpp: its own main, no Python, no GPU).  Exit status 0 and "failures": 0 when clean.
set -e
cd "$(dirname "$0")/.."
mkdir -p tests/_build
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I stark_mlwe_amd/csrc \
    tools/ntt_plan_check.cpp -o tests/_build/ntt_plan_check
./tests/_build/ntt_plan_check

#!/bin/bash
# tools/fri_mixed_sanitize.sh — AddressSanitizer + UBSan run of the stand-alone host check of the ragged commit phase, the classes and the passes of the
# mixed prove (tools/fri_mixed_check.cpp: its own main, no Python, no GPU).  Exit status 0 and "failures": 0 when clean.
set -e
cd "$(dirname "$0")/.."
mkdir -p tests/_build
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wno-unknown-pragmas -I stark_mlwe_amd/csrc \
    tools/fri_mixed_check.cpp -o tests/_build/fri_mixed_check
./tests/_build/fri_mixed_check

#!/bin/bash
# tools/merkle_climb_sanitize.sh — AddressSanitizer + UBSan run of the stand-alone host check of the Merkle climbs and the ragged plan
# (tools/merkle_climb_check.cpp: its own main, no Python, no GPU).  Exit status 0 and "failures": 0 when clean.
set -e
cd "$(dirname "$0")/.."
mkdir -p tests/_build
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wno-unknown-pragmas -I stark_mlwe_amd/csrc \
    tools/merkle_climb_check.cpp -o tests/_build/merkle_climb_check
./tests/_build/merkle_climb_check

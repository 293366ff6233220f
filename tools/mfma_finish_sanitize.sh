#!/bin/bash
# tools/mfma_finish_sanitize.sh — AddressSanitizer + UBSan run of the stand-alone host check of the matrix-core full rounds' residue tables and
# finishing step (tools/mfma_finish_check.cpp: its own main, no Python, no GPU).  Exit status 0 and "mismatches": 0 when clean.
set -e
cd "$(dirname "$0")/.."
mkdir -p tools/bin
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wno-misleading-indentation -I stark_mlwe_amd/csrc \
    tools/mfma_finish_check.cpp -o tools/bin/mfma_finish_check
./tools/bin/mfma_finish_check

#!/bin/sh
# TEST INFRASTRUCTURE: builds the CPU library behind tests/test_cc_diis.py (the DIIS bookkeeping of tf_cc_diis.h; no GPU code).
# "build.sh asan" builds the stand-alone program instead, with the address and undefined-behaviour sanitizers: run _build/cc_diis_asan.
set -e
cd "$(dirname "$0")"
mkdir -p _build
if [ "$1" = asan ]; then
    g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -DCC_DIIS_MAIN -o _build/cc_diis_asan cc_diis_model.cpp
else
    g++ -O2 -std=c++17 -shared -fPIC -Wall -o _build/libccdiis.so cc_diis_model.cpp
fi

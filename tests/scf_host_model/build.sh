#!/bin/sh
# TEST INFRASTRUCTURE: builds the CPU library behind tests/test_scf_host.py (the host arithmetic of tf_scf_host.h; no GPU code).
# "build.sh asan" builds the stand-alone program instead, with the address and undefined-behaviour sanitizers: run _build/scf_host_asan.
set -e
cd "$(dirname "$0")"
mkdir -p _build
if [ "$1" = asan ]; then
    g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -DSCF_HOST_MAIN -o _build/scf_host_asan scf_host_model.cpp
else
    g++ -O2 -std=c++17 -shared -fPIC -Wall -o _build/libscfhost.so scf_host_model.cpp
fi

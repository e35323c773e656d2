#!/bin/sh
# TEST INFRASTRUCTURE: builds the CPU library behind tests/test_ctx_plan.py (the owners of a context's lifetimes, the shard plans and
# the host tables of the device basis; no GPU code) and the owner checks as a stand-alone program: with AddressSanitizer and
# UndefinedBehaviorSanitizer where their runtime is installed (linked statically, so the program needs nothing of them where it runs;
# _build/owner_main.sanitized is written then), without them otherwise.
set -e
cd "$(dirname "$0")"
mkdir -p _build
g++ -O2 -std=c++17 -shared -fPIC -Wall -o _build/libctxmodel.so ctx_model.cpp ../../tuna_amd/csrc/tf_host.cpp
rm -f _build/owner_main _build/owner_main.sanitized
if g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -o _build/owner_main owner_main.cpp 2>/dev/null; then
    touch _build/owner_main.sanitized
else
    g++ -O1 -g -std=c++17 -Wall -o _build/owner_main owner_main.cpp
fi

#!/bin/sh
# TEST INFRASTRUCTURE: builds the CPU library behind tests/test_packed_tables.py (host tables of the packed layout; no GPU code)
set -e
cd "$(dirname "$0")"
mkdir -p _build
g++ -O2 -std=c++17 -shared -fPIC -Wall -o _build/libpackedtables.so packed_tables.cpp

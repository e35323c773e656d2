#!/bin/sh
# TEST INFRASTRUCTURE: builds the CPU library behind tests/test_excited_plan.py (the work-space plan of the excited-state and stability
# drivers; no GPU code)
set -e
cd "$(dirname "$0")"
mkdir -p _build
g++ -O2 -std=c++17 -shared -fPIC -Wall -o _build/libexcitedplan.so excited_plan.cpp

#!/bin/sh
# TEST INFRASTRUCTURE: builds the CPU library behind tests/test_xckernel_plan.py (the launch plan of the exchange-correlation kernel
# build; no GPU code)
set -e
cd "$(dirname "$0")"
mkdir -p _build
g++ -O2 -std=c++17 -shared -fPIC -Wall -o _build/libxckernelplan.so xckernel_plan.cpp

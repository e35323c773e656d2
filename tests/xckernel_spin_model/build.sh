#!/bin/sh
# TEST INFRASTRUCTURE: builds the CPU library behind tests/test_xckernel_spin_plan.py (the launch plan of the spin-blocked
# exchange-correlation kernel build; no GPU code)
set -e
cd "$(dirname "$0")"
mkdir -p _build
g++ -O2 -std=c++17 -shared -fPIC -Wall -o _build/libxckernelspinplan.so xckernel_spin_plan.cpp

# tests/hostsim/stamp_end.mk — the end of the 53-bit recency stamp under AddressSanitizer: the engine with a main() of its own
# (stamp_end_main.cpp), a stand-alone program; nothing is preloaded.  A make file of its own beside Makefile, which it leaves as it is:
#   make -C tests/hostsim -f stamp_end.mk stamp_end_asan [STAMP_END_OUT=<where>]      (tests/test_stamp_end_asan_cpu.py, then runs it)
R = ../..
C = $(R)/gubernator_amd/csrc
STAMP_END_OUT ?= /tmp/guber_stamp_end_asan
STAMP_END_DEPS = stamp_end.mk stamp_end_main.cpp fakehip/hip/hip_runtime.h fakehip/hip/hip_runtime_api_fake.h fakehip/fiber_runtime.h fakehip/hipcub/hipcub.hpp fakehip/rccl/rccl.h $(wildcard $(C)/*.h) $(wildcard $(C)/*.inl) $(C)/guber_engine.hip $(C)/guber_host.cpp $(C)/placement.cpp $(C)/worker_pool.cpp $(C)/wire.cpp $(R)/include/guber_gpu.h $(R)/include/guber_wire.h

.PHONY: stamp_end_asan
stamp_end_asan: $(STAMP_END_OUT)
$(STAMP_END_OUT): $(STAMP_END_DEPS)
	g++ -O1 -g -std=c++17 -fPIC -ffp-contract=off -fsanitize=address -Wno-attributes -Wno-unknown-pragmas -Wno-subobject-linkage -DGUBER_LAB -I fakehip -I $(R)/include -o $@ stamp_end_main.cpp $(C)/guber_host.cpp $(C)/placement.cpp $(C)/worker_pool.cpp $(C)/wire.cpp -lpthread -ldl

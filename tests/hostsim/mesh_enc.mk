# tests/hostsim/mesh_enc.mk — guber_wire_dev_eval_mesh_enc under AddressSanitizer: the engine with a main() of its own (mesh_enc_main.cpp), a
# stand-alone program; nothing is preloaded.  A make file of its own beside Makefile, which it leaves as it is:
#   make -C tests/hostsim -f mesh_enc.mk mesh_enc_asan [MESH_ENC_OUT=<where>]      (tests/test_mesh_enc_asan_cpu.py, then runs it)
R = ../..
C = $(R)/gubernator_amd/csrc
MESH_ENC_OUT ?= /tmp/guber_mesh_enc_asan
MESH_ENC_DEPS = mesh_enc.mk mesh_enc_main.cpp fakehip/hip/hip_runtime.h fakehip/hip/hip_runtime_api_fake.h fakehip/fiber_runtime.h fakehip/hipcub/hipcub.hpp fakehip/rccl/rccl.h $(wildcard $(C)/*.h) $(wildcard $(C)/*.inl) $(C)/guber_engine.hip $(C)/guber_host.cpp $(C)/placement.cpp $(C)/worker_pool.cpp $(C)/wire.cpp $(R)/include/guber_gpu.h $(R)/include/guber_wire.h

.PHONY: mesh_enc_asan
mesh_enc_asan: $(MESH_ENC_OUT)
$(MESH_ENC_OUT): $(MESH_ENC_DEPS)
	g++ -O1 -g -std=c++17 -fPIC -ffp-contract=off -fsanitize=address -Wno-attributes -Wno-unknown-pragmas -Wno-subobject-linkage -DGUBER_LAB -I fakehip -I $(R)/include -o $@ mesh_enc_main.cpp $(C)/guber_host.cpp $(C)/placement.cpp $(C)/worker_pool.cpp $(C)/wire.cpp -lpthread -ldl

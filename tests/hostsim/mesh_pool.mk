# tests/hostsim/mesh_pool.mk — guber_wire_mesh_pool_* under the sanitizers, as stand-alone programs; nothing is preloaded.  A make file of its
# own beside Makefile, which it leaves as it is:
#   make -C tests/hostsim -f mesh_pool.mk mesh_pool_asan [MESH_POOL_ASAN_OUT=<where>]   the engine with a main() of its own (mesh_pool_main.cpp) under
#                                                                                       AddressSanitizer (tests/test_mesh_pool_asan_cpu.py, then runs it)
#   make -C tests/hostsim -f mesh_pool.mk mesh_pool_tsan [MESH_POOL_TSAN_OUT=<where>]   guber_wire_mesh_pool.h alone against stand-ins for the decoder and the
#                                                                                       mesh (mesh_pool_tsan.cpp) under ThreadSanitizer (tests/test_mesh_pool_tsan_cpu.py)
R = ../..
C = $(R)/gubernator_amd/csrc
MESH_POOL_ASAN_OUT ?= /tmp/guber_mesh_pool_asan
MESH_POOL_TSAN_OUT ?= /tmp/guber_mesh_pool_tsan
MESH_POOL_DEPS = mesh_pool.mk mesh_pool_main.cpp fakehip/hip/hip_runtime.h fakehip/hip/hip_runtime_api_fake.h fakehip/fiber_runtime.h fakehip/hipcub/hipcub.hpp fakehip/rccl/rccl.h $(wildcard $(C)/*.h) $(wildcard $(C)/*.inl) $(C)/guber_engine.hip $(C)/guber_host.cpp $(C)/placement.cpp $(C)/worker_pool.cpp $(C)/wire.cpp $(R)/include/guber_gpu.h $(R)/include/guber_wire.h

.PHONY: mesh_pool_asan mesh_pool_tsan
mesh_pool_asan: $(MESH_POOL_ASAN_OUT)
$(MESH_POOL_ASAN_OUT): $(MESH_POOL_DEPS)
	g++ -O1 -g -std=c++17 -fPIC -ffp-contract=off -fsanitize=address -Wno-attributes -Wno-unknown-pragmas -Wno-subobject-linkage -DGUBER_LAB -I fakehip -I $(R)/include -o $@ mesh_pool_main.cpp $(C)/guber_host.cpp $(C)/placement.cpp $(C)/worker_pool.cpp $(C)/wire.cpp -lpthread -ldl

mesh_pool_tsan: $(MESH_POOL_TSAN_OUT)
$(MESH_POOL_TSAN_OUT): mesh_pool.mk mesh_pool_tsan.cpp wire_pool_tsan.cpp $(C)/guber_wire_mesh_pool.h $(C)/guber_wire_pool.h $(C)/guber_wire_parse.h $(C)/wire.cpp $(C)/guber_host.cpp $(R)/include/guber_wire.h $(R)/include/guber_gpu.h
	$(MAKE) -C $(R)/oracle
	g++ -O1 -g -std=c++17 -fsanitize=thread -I $(R)/include -o $@ mesh_pool_tsan.cpp $(C)/wire.cpp $(C)/guber_host.cpp -L$(R)/oracle -lguber_oracle -Wl,-rpath,$(abspath $(R)/oracle) -lpthread

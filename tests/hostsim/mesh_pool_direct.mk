# tests/hostsim/mesh_pool_direct.mk — the payload stage over a mesh with its direct path (guber_wire_mesh_pool.h + guber_wire_mesh_pool_direct.h) against
# stand-ins, under ThreadSanitizer: a stand-alone program, nothing is preloaded (tests/test_mesh_pool_direct_tsan_cpu.py).  A make file of its own
# beside Makefile and mesh_pool.mk, which it leaves as they are:
#   make -C tests/hostsim -f mesh_pool_direct.mk mesh_pool_direct_tsan [MESH_POOL_DIRECT_TSAN_OUT=<where>]
R = ../..
C = $(R)/gubernator_amd/csrc
MESH_POOL_DIRECT_TSAN_OUT ?= /tmp/guber_mesh_pool_direct_tsan

.PHONY: mesh_pool_direct_tsan
mesh_pool_direct_tsan: $(MESH_POOL_DIRECT_TSAN_OUT)
$(MESH_POOL_DIRECT_TSAN_OUT): mesh_pool_direct.mk mesh_pool_direct_tsan.cpp wire_pool_tsan.cpp $(C)/guber_wire_mesh_pool.h $(C)/guber_wire_mesh_pool_direct.h $(C)/guber_wire_pool.h $(C)/guber_wire_parse.h $(C)/wire.cpp $(C)/guber_host.cpp $(R)/include/guber_wire.h $(R)/include/guber_gpu.h
	$(MAKE) -C $(R)/oracle
	g++ -O1 -g -std=c++17 -fsanitize=thread -I $(R)/include -o $@ mesh_pool_direct_tsan.cpp $(C)/wire.cpp $(C)/guber_host.cpp -L$(R)/oracle -lguber_oracle -Wl,-rpath,$(abspath $(R)/oracle) -lpthread

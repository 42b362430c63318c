# builds the device tests of the entries stage's scan and of its further cases:  make -C tests/cpp -f entries_latency.mk
#   scantest              csrc/msm_block_scan.hpp by itself
#   entries_latency_test  entriestest.hip's checks over more cases (against libzkhip.so)
# gfx950 only; run by tests/test_gpu_msm_entries_latency.py on the GPU box
ROOT := ../..
all: scantest entries_latency_test
scantest: scantest.hip $(ROOT)/crypto3-zk_amd/csrc/msm_block_scan.hpp $(ROOT)/crypto3-zk_amd/csrc/zk_defs.hpp
	/opt/rocm/bin/hipcc --offload-arch=gfx950 -std=c++17 -O2 -Wno-unused-result -I $(ROOT)/crypto3-zk_amd/csrc scantest.hip -o $@
entries_latency_test: entries_latency_test.hip entriestest.hip $(wildcard $(ROOT)/crypto3-zk_amd/csrc/*.hpp) $(ROOT)/include/zkhip.h $(ROOT)/crypto3-zk_amd/libzkhip.so
	/opt/rocm/bin/hipcc --offload-arch=gfx950 -std=c++17 -O2 -Wno-unused-result -I $(ROOT)/crypto3-zk_amd/csrc entries_latency_test.hip -L $(ROOT)/crypto3-zk_amd -lzkhip -Wl,-rpath,'$$ORIGIN/../../crypto3-zk_amd' -o $@

# builds the device test of the MSM's entries stage (csrc/msm_entries.hpp) against libzkhip.so:  make -C tests/cpp -f entries.mk
#   entriestest  gfx950 only; run by tests/test_gpu_msm_entries.py on the GPU box
ROOT := ../..
all: entriestest
entriestest: entriestest.hip $(wildcard $(ROOT)/crypto3-zk_amd/csrc/*.hpp) $(ROOT)/include/zkhip.h $(ROOT)/crypto3-zk_amd/libzkhip.so
	/opt/rocm/bin/hipcc --offload-arch=gfx950 -std=c++17 -O2 -Wno-unused-result -I $(ROOT)/crypto3-zk_amd/csrc entriestest.hip -L $(ROOT)/crypto3-zk_amd -lzkhip -Wl,-rpath,'$$ORIGIN/../../crypto3-zk_amd' -o $@

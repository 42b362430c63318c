# builds the Pasta harnesses:  make -C tests/cpp -f pasta.mk
#   libarithdev_pasta.so  the device arithmetic of the Pallas / Vesta fields (arithdev_pasta.hip, the product's flags)
#   libpastatest.so       the shim over pallas / vesta (pasta_test.cpp, host compiler)
ROOT := ../..
SHIM_HDR := $(wildcard $(ROOT)/crypto3-zk_amd/include/nil/crypto3/zk/hip/*.hpp) $(ROOT)/include/zkhip.h
all: libarithdev_pasta.so libpastatest.so
libarithdev_pasta.so: arithdev_pasta.hip arithdev.hip $(ROOT)/crypto3-zk_amd/csrc/arith_ops.h $(wildcard $(ROOT)/crypto3-zk_amd/csrc/*.hpp)
	/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -shared -I $(ROOT)/crypto3-zk_amd/csrc arithdev_pasta.hip -o $@
libpastatest.so: pasta_test.cpp eval_polys_case.hpp fr_vector_case.hpp $(SHIM_HDR) $(wildcard $(ROOT)/crypto3-zk_amd/csrc/*.hpp) $(ROOT)/crypto3-zk_amd/libzkhip.so
	g++ -std=c++17 -O2 -fPIC -pthread -shared -I $(ROOT)/crypto3-zk_amd/include -I $(ROOT)/include pasta_test.cpp -L $(ROOT)/crypto3-zk_amd -lzkhip -Wl,-rpath,'$$ORIGIN/../../crypto3-zk_amd' -o $@

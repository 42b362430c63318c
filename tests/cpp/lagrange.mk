# builds the harness of the Lagrange-basis SRS:  make -C tests/cpp -f lagrange.mk
#   liblagrangetest.so  kimchi_pedersen_hip's add_lagrange_basis / commitment_evaluations over pallas / vesta (lagrange_test.cpp, host compiler)
ROOT := ../..
SHIM_HDR := $(wildcard $(ROOT)/crypto3-zk_amd/include/nil/crypto3/zk/hip/*.hpp) $(ROOT)/include/zkhip.h
all: liblagrangetest.so
liblagrangetest.so: lagrange_test.cpp $(SHIM_HDR) $(wildcard $(ROOT)/crypto3-zk_amd/csrc/*.hpp) $(ROOT)/crypto3-zk_amd/libzkhip.so
	g++ -std=c++17 -O2 -fPIC -pthread -shared -I $(ROOT)/crypto3-zk_amd/include -I $(ROOT)/include lagrange_test.cpp -L $(ROOT)/crypto3-zk_amd -lzkhip -Wl,-rpath,'$$ORIGIN/../../crypto3-zk_amd' -o $@

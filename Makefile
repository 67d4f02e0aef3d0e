PYTHON ?= python3
IMAGE  ?= ghcr.io/example/kata-xpu-device-plugin-amd:0.1.0

.PHONY: build build-hip test test-gpu bench soak image clean doctor validate burnin partition h2-selftest h2-selftest-asan

build:
	$(PYTHON) setup.py build_ext --inplace

build-hip:
	$(PYTHON) -c "from setup import build_hip; print(build_hip('gfx950'))"

test:
	$(PYTHON) -m pytest tests/ -q -m "not gpu"

# Stand-alone self-test of the native gRPC server's protocol code (HPACK,
# HTTP/2 framing and flow control, protobuf wire helpers). The -asan form
# checks the same program under AddressSanitizer + UBSan: host code only,
# run it on the CPU build machine.
h2-selftest:
	mkdir -p build
	$(CXX) -std=c++17 -O1 -g -Wall -Wextra -I native native/tests/h2_selftest.cpp -o build/h2_selftest
	./build/h2_selftest

h2-selftest-asan:
	mkdir -p build
	$(CXX) -std=c++17 -O1 -g -Wall -Wextra -fsanitize=address,undefined -fno-sanitize-recover=undefined \
		-I native native/tests/h2_selftest.cpp -o build/h2_selftest_asan
	./build/h2_selftest_asan

test-gpu:
	$(PYTHON) -m pytest tests/ -q -m gpu

bench:
	$(PYTHON) bench.py --steps 30 --warmup 5 --full

doctor:
	$(PYTHON) -m kata_xpu_device_plugin_amd.tools.doctor

validate:
	$(PYTHON) -m kata_xpu_device_plugin_amd.tools.validate

burnin:
	$(PYTHON) -m kata_xpu_device_plugin_amd.tools.burnin

partition:
	$(PYTHON) -m kata_xpu_device_plugin_amd.tools.partition show

soak:
	$(PYTHON) benchmarks/churn_soak.py --minutes 10 --clients 3

image:
	docker build -t $(IMAGE) .

clean:
	rm -rf build kata_xpu_device_plugin_amd/*.so kata_xpu_device_plugin_amd/**/__pycache__

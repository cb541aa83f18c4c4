// cli_host.h -- host-side tools of the `render` pipeline (cli_video.cpp) that know nothing about clips: the pool of encoder threads, the
// page-locked buffers recycled between a download and those threads, child processes started without a shell, a Y4M stream into a file or an
// encoder's stdin, and the removal of a directory of frames.
#pragma once

#include <dirent.h>
#include <fcntl.h>
#include <sys/wait.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>

#include "cli_common.h"

// Host threads that PNG-encode finished frames while the GPU traces the next ones.
class EncoderPool {
public:
    EncoderPool(int threads, size_t max_pending) : max_pending_(max_pending) {
        for (int k = 0; k < threads; ++k) workers_.emplace_back([this] { run(); });
    }
    ~EncoderPool() { finish(); }
    void submit(std::function<void()> job) {
        std::unique_lock<std::mutex> lock(mu_);
        space_.wait(lock, [&] { return jobs_.size() < max_pending_; });
        jobs_.push_back(std::move(job));
        work_.notify_one();
    }
    void finish() {
        {
            std::unique_lock<std::mutex> lock(mu_);
            done_ = true;
        }
        work_.notify_all();
        for (auto& t : workers_)
            if (t.joinable()) t.join();
    }

private:
    void run() {
        for (;;) {
            std::function<void()> job;
            {
                std::unique_lock<std::mutex> lock(mu_);
                work_.wait(lock, [&] { return done_ || !jobs_.empty(); });
                if (jobs_.empty()) return;
                job = std::move(jobs_.front());
                jobs_.pop_front();
                space_.notify_one();
            }
            job();
        }
    }
    std::mutex mu_;
    std::condition_variable work_, space_;
    std::deque<std::function<void()>> jobs_;
    std::vector<std::thread> workers_;
    size_t max_pending_;
    bool done_ = false;
};

// Page-locked frame buffers recycled between the download and the encoder threads.
class PinnedFrames {
public:
    PinnedFrames(size_t bytes, int count) {
        for (int k = 0; k < count; ++k) {
            void* p = nullptr;
            if (ptl_host_alloc(bytes, &p) != PTL_OK) break;
            all_.push_back(p);
            free_.push_back(p);
        }
    }
    ~PinnedFrames() {
        for (void* p : all_) ptl_host_free(p);
    }
    bool ok() const { return !all_.empty(); }
    uint8_t* take() {
        std::unique_lock<std::mutex> lock(mu_);
        cv_.wait(lock, [&] { return !free_.empty(); });
        void* p = free_.back();
        free_.pop_back();
        return static_cast<uint8_t*>(p);
    }
    void give(uint8_t* p) {
        std::unique_lock<std::mutex> lock(mu_);
        free_.push_back(p);
        cv_.notify_one();
    }

private:
    std::vector<void*> all_, free_;
    std::mutex mu_;
    std::condition_variable cv_;
};

// Start a program without a shell (arguments are passed as they are: no quoting rules to get wrong), as a fresh child process: `stdin_fd` >= 0
// becomes its stdin, `quiet` sends what it prints to /dev/null.  Its pid, or -1
inline pid_t start_program(const std::vector<std::string>& argv, int stdin_fd, bool quiet) {
    std::vector<char*> args;  // (built before the fork: the child only redirects and executes)
    for (const std::string& a : argv) args.push_back(const_cast<char*>(a.c_str()));
    args.push_back(nullptr);
    pid_t pid = fork();
    if (pid != 0) return pid;
    if (stdin_fd >= 0) dup2(stdin_fd, 0);  // (the copy is not close-on-exec)
    int null_fd = quiet ? open("/dev/null", O_WRONLY) : -1;
    if (null_fd >= 0) {
        dup2(null_fd, 1);
        dup2(null_fd, 2);
    }
    execvp(args[0], args.data());
    _exit(127);
}
inline int wait_program(pid_t pid) {  // its exit status; -1: it did not exit by itself
    int status = 0;
    return waitpid(pid, &status, 0) > 0 && WIFEXITED(status) ? WEXITSTATUS(status) : -1;
}
inline int run_program(const std::vector<std::string>& argv, bool quiet) {  // -1 = could not start
    pid_t pid = start_program(argv, -1, quiet);
    return pid < 0 ? -1 : wait_program(pid);
}

// One clip as a Y4M stream (--frames y4m): a file, or the stdin of an encoder started as a fresh child process.  Written by ONE thread
// in frame order; the first error sticks, later writes do nothing, and the clip loop looks at failed() before every frame -- a dead
// encoder ends the clip instead of blocking it (SIGPIPE is ignored in this mode: the write returns EPIPE).
class Y4mStream {
public:
    ~Y4mStream() { close(); }
    bool open_file(const std::string& path) {
        fd_ = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
        if (fd_ < 0) fail("cannot write `" + path + "`: " + std::strerror(errno));
        return fd_ >= 0;
    }
    bool open_program(const std::vector<std::string>& argv) {  // our pipe is its stdin
        int ends[2];
        if (::pipe2(ends, O_CLOEXEC) != 0) return fail("pipe: " + std::string(std::strerror(errno))), false;
        started_ = std::chrono::steady_clock::now();
        child_ = start_program(argv, ends[0], true);  // (the write end is close-on-exec, so the child sees the end of the stream)
        if (child_ < 0) {
            ::close(ends[0]);
            ::close(ends[1]);
            return fail("fork: " + std::string(std::strerror(errno))), false;
        }
        ::close(ends[0]);
        fd_ = ends[1];
        return true;
    }
    void write(const void* data, size_t n) {
        const char* p = static_cast<const char*>(data);
        while (n > 0 && !failed()) {
            ssize_t done = ::write(fd_, p, n);
            if (done < 0 && errno == EINTR) continue;
            if (done < 0) return fail(std::string(child_ > 0 ? "the encoder stopped reading the stream: " : "cannot write the stream: ") + std::strerror(errno));
            p += done;
            n -= (size_t)done;
        }
    }
    void fail(const std::string& what) {
        if (failed()) return;
        error_ = what;
        failed_.store(true, std::memory_order_release);
    }
    bool failed() const { return failed_.load(std::memory_order_acquire); }
    const std::string& error() const { return error_; }  // valid once failed()
    bool to_program() const { return child_ > 0; }
    double seconds() const { return seconds_since(started_); }
    // end of stream; for a child its exit status (-1: it did not exit by itself), for a file 0
    int close() {
        if (fd_ >= 0 && ::close(fd_) != 0) fail(std::string("cannot write the stream: ") + std::strerror(errno));
        fd_ = -1;
        return child_ > 0 ? wait_program(std::exchange(child_, -1)) : 0;
    }

private:
    int fd_ = -1;
    pid_t child_ = -1;
    std::atomic<bool> failed_{false};
    std::string error_;
    std::chrono::steady_clock::time_point started_ = std::chrono::steady_clock::now();
};

inline void remove_tree(const std::string& path) {  // rm -rf of a directory we created ourselves (frames only, one level)
    if (DIR* d = opendir(path.c_str())) {
        while (dirent* e = readdir(d)) {
            std::string name = e->d_name;
            if (name != "." && name != "..") ::unlink((path + "/" + name).c_str());
        }
        closedir(d);
    }
    ::rmdir(path.c_str());
}

/* oracle/mesa_runner.c -- draw a full-target quad with a given vertex + fragment shader on Mesa's
 * software rasteriser (llvmpipe), headless, through the DRI swrast interface.
 *
 * TEST INFRASTRUCTURE ONLY (see oracle/mesa.py).  The program holds no shader text: both texts, the
 * uniforms and the textures come from a job file.  Built on demand:  cc -O1 oracle/mesa_runner.c -ldl
 *
 * usage: mesa_runner <swrast_dri.so> <job file>
 * job file, one command per line, executed in order:
 *   program <vertex text file> <fragment text file>      compile + link + use
 *   target f32|u8 <w> <h>                                 FBO with a GL_RGBA32F / GL_RGBA8 texture
 *   texture <sampler uniform> <w> <h> <raw rgba8 file>    RGBA8, LINEAR, CLAMP_TO_EDGE, row 0 first, next unit
 *   uniform <name> <float|int|vec2|vec3|vec4|mat4> <hex bits> ...   (a name the linker dropped is skipped)
 *   draw <output file>                                    quad (0,0)-(w,h), Model = I, Projection = pixel
 *                                                         space -> NDC; raw readback (row 0 = image row 0)
 *                                                         is APPENDED to the output file
 * The first line of stdout is "GL_VERSION\tGL_RENDERER".
 */
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <GL/glcorearb.h>
#include <GL/internal/dri_interface.h>

static void die(const char *what, const char *detail) {
    fprintf(stderr, "mesa_runner: %s%s%s\n", what, detail ? ": " : "", detail ? detail : "");
    exit(2);
}

/* ---- loader callbacks: the drawable is never shown, all drawing goes to an FBO ---- */
static void get_drawable_info(__DRIdrawable *d, int *x, int *y, int *w, int *h, void *p) {
    (void)d, (void)p;
    *x = *y = 0;
    *w = *h = 16;
}
static void put_image(__DRIdrawable *d, int op, int x, int y, int w, int h, char *data, void *p) {
    (void)d, (void)op, (void)x, (void)y, (void)w, (void)h, (void)data, (void)p;
}
static void get_image(__DRIdrawable *d, int x, int y, int w, int h, char *data, void *p) {
    (void)d, (void)x, (void)y, (void)w, (void)h, (void)data, (void)p;
}
static void put_image2(__DRIdrawable *d, int op, int x, int y, int w, int h, int stride, char *data, void *p) {
    (void)d, (void)op, (void)x, (void)y, (void)w, (void)h, (void)stride, (void)data, (void)p;
}
static void get_image2(__DRIdrawable *d, int x, int y, int w, int h, int stride, char *data, void *p) {
    (void)d, (void)x, (void)y, (void)w, (void)h, (void)stride, (void)data, (void)p;
}
static const __DRIswrastLoaderExtension loader = {{__DRI_SWRAST_LOADER, 3}, get_drawable_info, put_image, get_image, put_image2, get_image2,
                                                  NULL, NULL, NULL, NULL};

/* ---- GL entry points ---- */
#define GL_FUNCTIONS(X)                                                                                                                      \
    X(PFNGLGETSTRINGPROC, glGetString) X(PFNGLGETERRORPROC, glGetError) X(PFNGLCREATESHADERPROC, glCreateShader)                               \
    X(PFNGLSHADERSOURCEPROC, glShaderSource) X(PFNGLCOMPILESHADERPROC, glCompileShader) X(PFNGLGETSHADERIVPROC, glGetShaderiv)                 \
    X(PFNGLGETSHADERINFOLOGPROC, glGetShaderInfoLog) X(PFNGLCREATEPROGRAMPROC, glCreateProgram) X(PFNGLATTACHSHADERPROC, glAttachShader)       \
    X(PFNGLBINDATTRIBLOCATIONPROC, glBindAttribLocation) X(PFNGLLINKPROGRAMPROC, glLinkProgram) X(PFNGLGETPROGRAMIVPROC, glGetProgramiv)       \
    X(PFNGLGETPROGRAMINFOLOGPROC, glGetProgramInfoLog) X(PFNGLUSEPROGRAMPROC, glUseProgram)                                                    \
    X(PFNGLGETUNIFORMLOCATIONPROC, glGetUniformLocation) X(PFNGLUNIFORM1FVPROC, glUniform1fv) X(PFNGLUNIFORM2FVPROC, glUniform2fv)             \
    X(PFNGLUNIFORM3FVPROC, glUniform3fv) X(PFNGLUNIFORM4FVPROC, glUniform4fv) X(PFNGLUNIFORM1IPROC, glUniform1i)                               \
    X(PFNGLUNIFORMMATRIX4FVPROC, glUniformMatrix4fv) X(PFNGLGENTEXTURESPROC, glGenTextures) X(PFNGLBINDTEXTUREPROC, glBindTexture)             \
    X(PFNGLACTIVETEXTUREPROC, glActiveTexture) X(PFNGLTEXIMAGE2DPROC, glTexImage2D) X(PFNGLTEXPARAMETERIPROC, glTexParameteri)                 \
    X(PFNGLGENFRAMEBUFFERSPROC, glGenFramebuffers) X(PFNGLBINDFRAMEBUFFERPROC, glBindFramebuffer)                                              \
    X(PFNGLFRAMEBUFFERTEXTURE2DPROC, glFramebufferTexture2D) X(PFNGLCHECKFRAMEBUFFERSTATUSPROC, glCheckFramebufferStatus)                      \
    X(PFNGLVIEWPORTPROC, glViewport) X(PFNGLDISABLEPROC, glDisable) X(PFNGLCLEARCOLORPROC, glClearColor) X(PFNGLCLEARPROC, glClear)            \
    X(PFNGLGENVERTEXARRAYSPROC, glGenVertexArrays) X(PFNGLBINDVERTEXARRAYPROC, glBindVertexArray) X(PFNGLGENBUFFERSPROC, glGenBuffers)         \
    X(PFNGLBINDBUFFERPROC, glBindBuffer) X(PFNGLBUFFERDATAPROC, glBufferData) X(PFNGLENABLEVERTEXATTRIBARRAYPROC, glEnableVertexAttribArray)   \
    X(PFNGLVERTEXATTRIBPOINTERPROC, glVertexAttribPointer) X(PFNGLDRAWARRAYSPROC, glDrawArrays) X(PFNGLFINISHPROC, glFinish)                   \
    X(PFNGLPIXELSTOREIPROC, glPixelStorei) X(PFNGLREADPIXELSPROC, glReadPixels)
#define DECLARE(type, name) static type name;
GL_FUNCTIONS(DECLARE)

static char *read_file(const char *path, long *size) {
    FILE *f = fopen(path, "rb");
    if (!f) die("cannot open", path);
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    char *buf = malloc(n + 1);
    if (fread(buf, 1, n, f) != (size_t)n) die("short read", path);
    buf[n] = 0;
    fclose(f);
    if (size) *size = n;
    return buf;
}

static void check_gl(const char *where) {
    GLenum e = glGetError();
    if (e != GL_NO_ERROR) {
        char msg[64];
        snprintf(msg, sizeof msg, "GL error 0x%04x", e);
        die(where, msg);
    }
}

static GLuint compile(GLenum kind, const char *path) {
    char *text = read_file(path, NULL);
    GLuint s = glCreateShader(kind);
    glShaderSource(s, 1, (const GLchar *const *)&text, NULL);
    glCompileShader(s);
    GLint ok = 0;
    glGetShaderiv(s, GL_COMPILE_STATUS, &ok);
    if (!ok) {
        static char log[1 << 16];
        glGetShaderInfoLog(s, sizeof log, NULL, log);
        die(path, log);
    }
    free(text);
    return s;
}

int main(int argc, char **argv) {
    if (argc != 3) die("usage: mesa_runner <swrast_dri.so> <job file>", NULL);
    void *glapi = dlopen("libglapi.so.0", RTLD_NOW | RTLD_GLOBAL);
    if (!glapi) die("dlopen libglapi.so.0", dlerror());
    void *drv = dlopen(argv[1], RTLD_NOW | RTLD_GLOBAL);
    if (!drv) die("dlopen driver", dlerror());
    const __DRIextension **(*get_exts)(void) = (const __DRIextension **(*)(void))dlsym(drv, __DRI_DRIVER_GET_EXTENSIONS "_swrast");
    if (!get_exts) die("no " __DRI_DRIVER_GET_EXTENSIONS "_swrast", NULL);
    const __DRIextension **exts = get_exts();
    const __DRIcoreExtension *core = NULL;
    const __DRIswrastExtension *swrast = NULL;
    for (int i = 0; exts[i]; i++) {
        if (!strcmp(exts[i]->name, __DRI_CORE) && exts[i]->version >= 2) core = (const __DRIcoreExtension *)exts[i];
        if (!strcmp(exts[i]->name, __DRI_SWRAST) && exts[i]->version >= 4) swrast = (const __DRIswrastExtension *)exts[i];
    }
    if (!core || !swrast) die("driver lacks DRI_Core v2 / DRI_SWRast v4", NULL);
    const __DRIextension *loader_exts[] = {&loader.base, NULL};
    const __DRIconfig **configs = NULL;
    __DRIscreen *screen = swrast->createNewScreen2(0, loader_exts, exts, &configs, NULL);
    if (!screen || !configs || !configs[0]) die("createNewScreen2 failed", NULL);
    const uint32_t attribs[] = {__DRI_CTX_ATTRIB_MAJOR_VERSION, 3, __DRI_CTX_ATTRIB_MINOR_VERSION, 0};
    unsigned err = 0;
    __DRIcontext *ctx = swrast->createContextAttribs(screen, __DRI_API_GLES3, configs[0], NULL, 2, attribs, &err, NULL);
    if (!ctx) die("createContextAttribs(GLES 3.0) failed", NULL);
    __DRIdrawable *drawable = swrast->createNewDrawable(screen, configs[0], NULL);
    if (!drawable || !core->bindContext(ctx, drawable, drawable)) die("bindContext failed", NULL);

    void *(*get_proc)(const char *) = (void *(*)(const char *))dlsym(glapi, "_glapi_get_proc_address");
    if (!get_proc) die("no _glapi_get_proc_address", NULL);
#define LOAD(type, name)              \
    name = (type)get_proc(#name);     \
    if (!name) die("no entry point", #name);
    GL_FUNCTIONS(LOAD)
    printf("%s\t%s\n", (const char *)glGetString(GL_VERSION), (const char *)glGetString(GL_RENDERER));
    fflush(stdout);

    GLuint vao, vbo, program = 0;
    glGenVertexArrays(1, &vao);
    glBindVertexArray(vao);
    glGenBuffers(1, &vbo);
    glBindBuffer(GL_ARRAY_BUFFER, vbo);
    glDisable(GL_DEPTH_TEST);
    glDisable(GL_BLEND);
    glDisable(GL_DITHER);
    glDisable(GL_CULL_FACE);
    glPixelStorei(GL_PACK_ALIGNMENT, 1);
    glPixelStorei(GL_UNPACK_ALIGNMENT, 1);

    int width = 0, height = 0, is_float = 1, unit = 0;
    long job_size;
    char *job = read_file(argv[2], &job_size);
    for (char *line = strtok(job, "\n"); line; line = strtok(NULL, "\n")) {
        char a[1024], b[1024], c[1024];
        int n1, n2, used = 0;
        if (sscanf(line, "program %1023s %1023s", a, b) == 2) {
            program = glCreateProgram();
            glAttachShader(program, compile(GL_VERTEX_SHADER, a));
            glAttachShader(program, compile(GL_FRAGMENT_SHADER, b));
            glBindAttribLocation(program, 0, "position");
            glLinkProgram(program);
            GLint ok = 0;
            glGetProgramiv(program, GL_LINK_STATUS, &ok);
            if (!ok) {
                static char log[1 << 16];
                glGetProgramInfoLog(program, sizeof log, NULL, log);
                die("link", log);
            }
            glUseProgram(program);
            check_gl("program");
        } else if (sscanf(line, "target %1023s %d %d", a, &n1, &n2) == 3) {
            GLuint tex, fbo;
            width = n1, height = n2, is_float = !strcmp(a, "f32");
            glGenTextures(1, &tex);
            glActiveTexture(GL_TEXTURE0 + 31);
            glBindTexture(GL_TEXTURE_2D, tex);
            glTexImage2D(GL_TEXTURE_2D, 0, is_float ? GL_RGBA32F : GL_RGBA8, width, height, 0, GL_RGBA, is_float ? GL_FLOAT : GL_UNSIGNED_BYTE, NULL);
            glTexParameteri(GL_TEXTURE_2D, GL_TEXTURE_MIN_FILTER, GL_NEAREST);
            glTexParameteri(GL_TEXTURE_2D, GL_TEXTURE_MAG_FILTER, GL_NEAREST);
            glGenFramebuffers(1, &fbo);
            glBindFramebuffer(GL_FRAMEBUFFER, fbo);
            glFramebufferTexture2D(GL_FRAMEBUFFER, GL_COLOR_ATTACHMENT0, GL_TEXTURE_2D, tex, 0);
            if (glCheckFramebufferStatus(GL_FRAMEBUFFER) != GL_FRAMEBUFFER_COMPLETE) die("framebuffer incomplete", a);
            glViewport(0, 0, width, height);
            check_gl("target");
        } else if (sscanf(line, "texture %1023s %d %d %1023s", a, &n1, &n2, b) == 4) {
            long size;
            char *texels = read_file(b, &size);
            if (size != 4L * n1 * n2) die("texture file size", b);
            GLuint tex;
            glGenTextures(1, &tex);
            glActiveTexture(GL_TEXTURE0 + unit);
            glBindTexture(GL_TEXTURE_2D, tex);
            glTexImage2D(GL_TEXTURE_2D, 0, GL_RGBA8, n1, n2, 0, GL_RGBA, GL_UNSIGNED_BYTE, texels);
            glTexParameteri(GL_TEXTURE_2D, GL_TEXTURE_MIN_FILTER, GL_LINEAR);
            glTexParameteri(GL_TEXTURE_2D, GL_TEXTURE_MAG_FILTER, GL_LINEAR);
            glTexParameteri(GL_TEXTURE_2D, GL_TEXTURE_WRAP_S, GL_CLAMP_TO_EDGE);
            glTexParameteri(GL_TEXTURE_2D, GL_TEXTURE_WRAP_T, GL_CLAMP_TO_EDGE);
            GLint loc = glGetUniformLocation(program, a);
            if (loc >= 0) glUniform1i(loc, unit);
            unit++;
            free(texels);
            check_gl("texture");
        } else if (sscanf(line, "uniform %1023s %1023s %n", a, b, &used) == 2 && used) {
            union { uint32_t u; float f; int32_t i; } v[16];
            int count = 0;
            for (char *p = line + used, *end; count < 16; p = end, count++) {
                v[count].u = (uint32_t)strtoul(p, &end, 16);
                if (end == p) break;
            }
            int want = !strcmp(b, "mat4") ? 16 : !strcmp(b, "vec4") ? 4 : !strcmp(b, "vec3") ? 3 : !strcmp(b, "vec2") ? 2 : 1;
            if (count != want) die("uniform value count", line);
            GLint loc = glGetUniformLocation(program, a);
            if (loc < 0) continue;
            if (!strcmp(b, "int")) glUniform1i(loc, v[0].i);
            else if (!strcmp(b, "float")) glUniform1fv(loc, 1, &v[0].f);
            else if (!strcmp(b, "vec2")) glUniform2fv(loc, 1, &v[0].f);
            else if (!strcmp(b, "vec3")) glUniform3fv(loc, 1, &v[0].f);
            else if (!strcmp(b, "vec4")) glUniform4fv(loc, 1, &v[0].f);
            else if (!strcmp(b, "mat4")) glUniformMatrix4fv(loc, 1, GL_FALSE, &v[0].f);
            else die("uniform type", b);
            check_gl(line);
        } else if (sscanf(line, "draw %1023s", c) == 1) {
            if (!program || !width) die("draw before program / target", NULL);
            const float w = (float)width, h = (float)height;
            const float quad[18] = {0, 0, 0, w, 0, 0, w, h, 0, 0, 0, 0, w, h, 0, 0, h, 0};
            const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
            const float projection[16] = {2 / w, 0, 0, 0, 0, 2 / h, 0, 0, 0, 0, 1, 0, -1, -1, 0, 1};
            GLint loc;
            if ((loc = glGetUniformLocation(program, "Model")) >= 0) glUniformMatrix4fv(loc, 1, GL_FALSE, identity);
            if ((loc = glGetUniformLocation(program, "Projection")) >= 0) glUniformMatrix4fv(loc, 1, GL_FALSE, projection);
            glBufferData(GL_ARRAY_BUFFER, sizeof quad, quad, GL_STATIC_DRAW);
            glEnableVertexAttribArray(0);
            glVertexAttribPointer(0, 3, GL_FLOAT, GL_FALSE, 0, NULL);
            glClearColor(0, 0, 0, 0);
            glClear(GL_COLOR_BUFFER_BIT);
            glDrawArrays(GL_TRIANGLES, 0, 6);
            glFinish();
            size_t bytes = (size_t)width * height * 4 * (is_float ? 4 : 1);
            void *pixels = malloc(bytes);
            glReadPixels(0, 0, width, height, GL_RGBA, is_float ? GL_FLOAT : GL_UNSIGNED_BYTE, pixels);
            check_gl("draw");
            FILE *f = fopen(c, "ab");
            if (!f || fwrite(pixels, 1, bytes, f) != bytes) die("cannot write", c);
            fclose(f);
            free(pixels);
        } else if (line[0] && line[0] != '#') {
            die("bad job line", line);
        }
    }
    fflush(stdout);
    return 0;
}

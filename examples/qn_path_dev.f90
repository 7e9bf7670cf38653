!  qn_path_dev -- driver_dev's loop (the reference's test/driver2.f90:66-195 on device buffers, the library's built-in
!  separable bounded quadratic, classic entry setulb_dev) to a NEW_X return, then the model on the free variables
!  over a range of shifts: one lbfgsb_kkt pass at the last iterate, the rows it reports at a bound (codes 1, 2, 3)
!  pinned by lbfgsb_qn_path_set, the curve log det (B_FF + mu I) at 5 shifts (lbfgsb_qn_path_logdet: host only), and
!  the trust-region step -(B_FF + mu I)^-1 g_F of the gradient at this iterate with radius half the Newton step's
!  length (lbfgsb_qn_path_solve for that length, lbfgsb_qn_path_trust).
!
!     qn_path_dev [n [m [iterations]]]      defaults 100000, 5, 12
!
!  Output: one "Iterate" line per iterate, then
!     QNPATH col = <stored pairs> pinned = <pinned rows>
!     QNPATH logdet <mu> <log det (B_FF + mu I)> <info>            (5 lines)
!     QNPATH newton <||(B_FF)^-1 g_F||> <g'(B_FF)^-1 g>
!     QNPATH trust <mu> <||step||> <predicted decrease> <on_boundary> <evaluations>
!     QNPATH step <sum of the step's entries> <sum of their absolute values> <largest |step| on a pinned row>
      program qn_path_dev

      use lbfgsb_module, wp => lbfgsp_wp
      use iso_c_binding
      use iso_fortran_env, only: output_unit

      implicit none

      interface
         function hipMalloc(ptr, nbytes) bind(C, name='hipMalloc') result(rc)
            import :: c_ptr, c_size_t, c_int
            type(c_ptr) :: ptr
            integer(c_size_t), value :: nbytes
            integer(c_int) :: rc
         end function hipMalloc
         function hipFree(ptr) bind(C, name='hipFree') result(rc)
            import :: c_ptr, c_int
            type(c_ptr), value :: ptr
            integer(c_int) :: rc
         end function hipFree
         function hipMemcpy(dst, src, nbytes, kind) bind(C, name='hipMemcpy') result(rc)
            import :: c_ptr, c_size_t, c_int
            type(c_ptr), value :: dst, src
            integer(c_size_t), value :: nbytes
            integer(c_int), value :: kind
            integer(c_int) :: rc
         end function hipMemcpy
         function hipMemset(dst, val, nbytes) bind(C, name='hipMemset') result(rc)
            import :: c_ptr, c_size_t, c_int
            type(c_ptr), value :: dst
            integer(c_int), value :: val
            integer(c_size_t), value :: nbytes
            integer(c_int) :: rc
         end function hipMemset
      end interface
      integer(c_int), parameter :: H2D = 1, D2H = 2
      integer, parameter    :: NMU = 5

      integer               :: n, m, maxit, rc, i, iters
      real(wp), parameter   :: factr = 0.0_wp, pgtol = 0.0_wp
      character(len=60)     :: task, csave
      character(len=32)     :: arg
      logical               :: lsave(4)
      integer               :: isave(44)
      real(wp)              :: f, dsave(29)
      real(c_double)        :: mus(NMU), logdet(NMU), mu0(1), norm2(1), vx(1), res(4), ssum, sabs, spin
      integer(c_int32_t)    :: info(NMU)
      type(c_ptr)           :: ctx, dx, dg, dl, du, dnbd, dstep, dstatus
      integer(c_int8_t), allocatable, target :: hstatus(:)
      integer(c_int64_t)    :: cnt(LBFGSB_KKT_NCNT), pinned
      real(c_double)        :: val(LBFGSB_KKT_NVAL)
      real(wp), allocatable, target :: hbuf(:)
      integer(c_int32_t), allocatable, target :: hnbd(:)
      integer(c_size_t)     :: vbytes

      n = 100000; m = 5; maxit = 12
      if (command_argument_count() >= 1) then
         call get_command_argument(1, arg); read (arg, *) n
      end if
      if (command_argument_count() >= 2) then
         call get_command_argument(2, arg); read (arg, *) m
      end if
      if (command_argument_count() >= 3) then
         call get_command_argument(3, arg); read (arg, *) maxit
      end if

      vbytes = int(n, c_size_t)*int(storage_size(1.0_wp)/8, c_size_t)
      call chk(hipMalloc(dx, vbytes), 'hipMalloc x')
      call chk(hipMalloc(dg, vbytes), 'hipMalloc g')
      call chk(hipMalloc(dl, vbytes), 'hipMalloc l')
      call chk(hipMalloc(du, vbytes), 'hipMalloc u')
      call chk(hipMalloc(dstep, vbytes), 'hipMalloc step')
      call chk(hipMalloc(dstatus, int(n, c_size_t)), 'hipMalloc status')
      call chk(hipMalloc(dnbd, int(n, c_size_t)*4_c_size_t), 'hipMalloc nbd')
      call chk(hipMemset(dx, 0_c_int, vbytes), 'hipMemset x')             ! x0 = 0
      call chk(hipMemset(dg, 0_c_int, vbytes), 'hipMemset g')
      allocate (hbuf(n))
      hbuf = -1.0_wp                                                       ! l = -1
      call chk(hipMemcpy(dl, c_loc(hbuf), vbytes, H2D), 'hipMemcpy l')
      hbuf = 1.0_wp                                                        ! u = +1
      call chk(hipMemcpy(du, c_loc(hbuf), vbytes, H2D), 'hipMemcpy u')
      allocate (hnbd(n))
      do i = 1, n
         hnbd(i) = int(mod(i, 4), c_int32_t)                               ! all four bound types
      end do
      call chk(hipMemcpy(dnbd, c_loc(hnbd), int(n, c_size_t)*4_c_size_t, H2D), 'hipMemcpy nbd')
      deallocate (hnbd)

      call lbfgsb_create(ctx, n, m, 0, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_create failed: ', lbfgsb_error_message()
         error stop 1
      end if

      task = 'START'
      f = 0.0_wp
      do while (task(1:2) == 'FG' .or. task == 'NEW_X' .or. task == 'START')
         call setulb_dev(ctx, dx, dl, du, dnbd, f, dg, factr, pgtol, task, -1, csave, lsave, isave, dsave, rc)
         if (rc /= 0) then
            write (output_unit, '(2a)') ' setulb_dev failed: ', lbfgsb_error_message()
            error stop 1
         end if
         if (task(1:2) == 'FG') then
            call lbfgsb_objective(ctx, 0, dx, dg, rc, f)
            if (rc /= 0) error stop 2
         else if (task(1:5) == 'NEW_X') then
            write (output_unit, '(2(a,i5,4x),a,1p,d12.5,4x,a,1p,d12.5)') 'Iterate', isave(30), 'nfg =', isave(34), &
               'f =', f, '|proj g| =', dsave(13)
            if (isave(30) >= maxit) exit                                   ! the model of this NEW_X return
         end if
      end do

      ! the rows at a bound at this iterate (codes 1, 2, 3 of lbfgsb_kkt's status: mask 0b11100) are pinned
      call lbfgsb_kkt(ctx, dx, dl, du, dnbd, dg, 0.0_c_double, c_null_ptr, c_null_ptr, dstatus, cnt, val, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_kkt failed: ', lbfgsb_error_message()
         error stop 1
      end if
      call lbfgsb_qn_path_set(ctx, dstatus, 28, pinned, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_qn_path_set failed: ', lbfgsb_error_message()
         error stop 1
      end if
      write (output_unit, '(a,i4,a,i0)') 'QNPATH col =', isave(28), ' pinned = ', pinned
      ! the log det curve: host only, no pass
      mus = [0.0_c_double, 0.1_c_double, 1.0_c_double, 10.0_c_double, 100.0_c_double]
      call lbfgsb_qn_path_logdet(ctx, NMU, mus, logdet, info, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_qn_path_logdet failed: ', lbfgsb_error_message()
         error stop 1
      end if
      do i = 1, NMU
         write (output_unit, '(a,2es25.16e3,i3)') 'QNPATH logdet', mus(i), logdet(i), info(i)
      end do
      ! the length of the Newton step of the free variables (the read pass alone), then the trust step at half of it
      mu0 = 0.0_c_double
      call lbfgsb_qn_path_solve(ctx, dg, 1, mu0, c_null_ptr, n, norm2, vx, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_qn_path_solve failed: ', lbfgsb_error_message()
         error stop 1
      end if
      write (output_unit, '(a,2es25.16e3)') 'QNPATH newton', sqrt(norm2(1)), vx(1)
      call lbfgsb_qn_path_trust(ctx, dg, 0.5_c_double*sqrt(norm2(1)), 0.0_c_double, 0, dstep, res, iters, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_qn_path_trust failed: ', lbfgsb_error_message()
         error stop 1
      end if
      write (output_unit, '(a,3es25.16e3,2i4)') 'QNPATH trust', res(1), res(2), res(3), int(res(4)), iters
      allocate (hstatus(n))
      call chk(hipMemcpy(c_loc(hstatus), dstatus, int(n, c_size_t), D2H), 'hipMemcpy status')
      call chk(hipMemcpy(c_loc(hbuf), dstep, vbytes, D2H), 'hipMemcpy step')
      ssum = 0.0_c_double; sabs = 0.0_c_double; spin = 0.0_c_double
      do i = 1, n
         ssum = ssum + real(hbuf(i), c_double)
         sabs = sabs + abs(real(hbuf(i), c_double))
         if (hstatus(i) >= 1_c_int8_t) spin = max(spin, abs(real(hbuf(i), c_double)))
      end do
      write (output_unit, '(a,3es25.16e3)') 'QNPATH step', ssum, sabs, spin
      deallocate (hstatus, hbuf)

      task = 'STOP: QN_PATH_DEV'
      call lbfgsb_destroy(ctx)
      rc = hipFree(dx); rc = hipFree(dg); rc = hipFree(dl); rc = hipFree(du)
      rc = hipFree(dstep); rc = hipFree(dnbd); rc = hipFree(dstatus)

      contains

      subroutine chk(code, what)
      integer(c_int), intent(in) :: code
      character(len=*), intent(in) :: what
      if (code /= 0) then
         write (output_unit, '(3a,i0)') ' ', what, ' failed, hipError ', code
         error stop 3
      end if
      end subroutine chk

      end program qn_path_dev
